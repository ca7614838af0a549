"""tests/guards.py on host tensors: three toy operators that are wrong in the three ways the guards exist for must
each be reported, a correct one must pass, and the patch must be gone after the block."""
import pytest
import torch

import guards

HERE = (__name__,)       # the module filter, widened to this file; any_device=True admits host tensors


def _past(t, k):
    """The element k places past the end of the contiguous tensor `t`, the way a kernel with a raw pointer sees it."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + t.numel() - 1 + k)


def op_ok(x):
    out = torch.empty_like(x)
    ws = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
    ws.copy_(x.reshape(-1))
    out.copy_(ws.view_as(x) * 2)
    return out


def op_skips_last(x):
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    out.view(-1)[:-1] = x.reshape(-1)[:-1] * 2
    return out


def op_writes_past(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    _past(out, 1).fill_(7.0)
    return out


def op_reads_workspace(x):
    ws = torch.empty(x.numel() + 1, dtype=torch.float32, device=x.device)
    ws[:-1] = x.reshape(-1)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    out.copy_(ws.sum() * 0.0 + x.sum())        # the unwritten word times zero: harmless unless it is a NaN or an Inf
    return out


def op_ids(n):
    ids = torch.empty(n, dtype=torch.int64)
    ids[:-1] = 0
    return ids


def _x():
    return torch.arange(15, dtype=torch.float32).reshape(3, 5)


def _armed(p):
    return guards.armed(p, modules=HERE, any_device=True)


def test_patterns_are_what_they_claim():
    for dt in (torch.float32, torch.float16):
        va, wa = guards.pattern_word("A", dt)
        vb, wb = guards.pattern_word("B", dt)
        a = torch.tensor([wa], dtype=va).view(dt)
        b = torch.tensor([wb], dtype=vb).view(dt)
        assert bool(torch.isnan(a).all()) and bool(torch.isfinite(b).all())
    assert guards.pattern_word("A", torch.float32)[1] & 0xFFFFFFFF == 0x7FE5A5A5
    assert guards.pattern_word("B", torch.float32)[1] & 0xFFFFFFFF == 0x7F7FA5A5
    assert guards.pattern_word("A", torch.float16)[1] & 0xFFFF == 0x7EA5
    assert guards.pattern_word("B", torch.float16)[1] & 0xFFFF == 0x7BA5
    for p in "AB":      # no positive integer poison: an id read by mistake is rejected, not dereferenced
        for dt in (torch.int32, torch.int64, torch.int16):
            assert guards.pattern_word(p, dt)[1] < 0
    assert guards.pattern_word("A", torch.uint8) == (torch.uint8, 0xA5)
    assert guards.pattern_word("B", torch.uint8) == (torch.uint8, 0xC3)
    assert guards.PAD_BYTES == 64 * 1024 and guards.PAD_BYTES % 256 == 0


def test_correct_operator_passes():
    x = _x()
    plain = op_ok(x)
    for p in "AB":
        with _armed(p) as g:
            out = op_ok(x)
        g.check()
        assert g.unwritten() == {}
        assert guards.same_bits(out, plain)
        assert out.is_contiguous() and out.shape == x.shape
        assert out.data_ptr() % 256 == g.records[0].base.data_ptr() % 256     # PAD keeps the base's alignment
        assert len(g.records) == 2
        assert g.sites() == ["test_guards.py:op_ok:out", "test_guards.py:op_ok:ws"]
        assert g.records[0].site.startswith("test_guards.py:")


def test_unwritten_element_is_reported():
    x = _x()
    for p in "AB":
        with _armed(p) as g:
            op_skips_last(x)
        g.check()
        left = g.unwritten()
        assert list(left.values()) == [1], left
        assert "test_guards.py:op_skips_last:out" in next(iter(left))
        # ... unless that very allocation is unwritten by contract
        assert g.unwritten(allowed={"test_guards.py:op_skips_last:out": "toy"}) == {}
    with _armed("A") as g:      # integers too
        op_ids(9)
    assert list(g.unwritten().values()) == [1]


def test_write_past_the_end_is_reported():
    x = _x()
    for p in "AB":
        with _armed(p) as g:
            op_writes_past(x)
        bad = g.broken_fences()
        assert len(bad) == 1 and "op_writes_past:out" in bad[0] and "past the end" in bad[0], bad
        with pytest.raises(AssertionError, match="op_writes_past"):
            g.check()
        assert g.unwritten() == {}


def test_unwritten_workspace_word_shows_between_patterns():
    """The workspace is exempt from unwritten() (an operator need not fill its scratch) but not from independence:
    the result differs between the plain run and pattern A, which is how a guard case reports it."""
    x = _x()
    ws_like = torch.empty(x.numel(), dtype=torch.uint8)
    plain = op_reads_workspace(x)
    res = {}
    for p in "AB":
        with _armed(p) as g:
            res[p] = op_reads_workspace(x)
            scratch = torch.empty(x.numel(), dtype=torch.uint8, device=ws_like.device)     # a workspace, never written
        g.check()
        left = g.unwritten()      # the float scratch is reported, the uint8 one exempt
        assert any("op_reads_workspace:ws" in k for k in left) and not any("scratch" in k for k in left)
        # (under A the result is reported too: the poison NaN keeps its payload through the arithmetic)
        assert len(left) == (2 if p == "A" else 1), left
    assert not guards.same_bits(res["A"], plain) and bool(torch.isnan(res["A"]))
    assert guards.same_bits(res["B"], plain)            # finite poison times zero: why there are two patterns

    def case(inp):
        return {"out": op_reads_workspace(inp(x))}
    with mock_filter():
        with pytest.raises(AssertionError, match="differs between the plain run and the A run"):
            guards.run_case(case, reset=lambda: None, allowed={"test_guards.py:op_reads_workspace:ws": "toy"})
        guards.run_case(lambda inp: {"out": op_ok(inp(x))}, reset=lambda: None)


class mock_filter:
    """run_case arms with the default filter: widen it for the toys."""

    def __enter__(self):
        self.real = guards.armed
        guards.armed = lambda p: self.real(p, modules=HERE, any_device=True)

    def __exit__(self, *exc):
        guards.armed = self.real


def test_filter_passes_everything_else_through():
    x = _x()
    with guards.armed("A") as g:                       # default filter: this module is not the package
        op_skips_last(x)
    assert g.records == []
    with guards.armed("A", modules=HERE) as g:         # our module, but a host tensor
        op_skips_last(x)
    assert g.records == []
    with _armed("A") as g:
        t = torch.empty(4, pin_memory=False)
        assert len(g.records) == 1 and t.shape == (4,)
        torch.empty((2, 3), dtype=torch.int32)
        torch.empty(2, 3, dtype=torch.float16)
        torch.empty(size=(0, 3))
        assert [r.shape for r in g.records[1:]] == [(2, 3), (2, 3), (0, 3)]
        assert [r.dtype for r in g.records[1:]] == [torch.int32, torch.float16, torch.float32]
    g.check()


def test_fenced_input():
    x = _x().requires_grad_(True)
    g = guards.Guard("A")
    f = g.fenced(x)
    assert f.requires_grad and f.is_leaf and f.is_contiguous() and guards.same_bits(f, x)
    assert bool(torch.isnan(_past(f.detach(), 1)).all())
    (f * 2).sum().backward()
    assert guards.same_bits(f.grad, torch.full_like(x, 2.0))
    g.check()
    assert guards.same_bits(guards.fenced(x.detach().t()), x.detach().t().contiguous())
    with pytest.raises(TypeError):
        guards.fenced(torch.zeros(3, dtype=torch.int64))


def test_patch_is_restored():
    real = (torch.empty, torch.empty_like)
    with _armed("A"):
        assert torch.empty is not real[0] and torch.empty_like is not real[1]
    assert (torch.empty, torch.empty_like) == real
    with pytest.raises(KeyError):
        with _armed("B"):
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like) == real
    with pytest.raises(ValueError):
        with guards.armed("C"):
            pass
    assert (torch.empty, torch.empty_like) == real


def test_allowed_names_single_allocations():
    for name, why in guards.ALLOWED.items():
        f, func, target = name.split(":")
        assert f.endswith(".py") and func and target and not target.startswith("line"), name
        assert ".hip" in why, "the reason cites the kernel: %s" % name
