"""The face-list and topology memos (ops/base.py `_FACES`; pytorch3d_shim/structures.py `_FACES_PACKED_CACHE`, `_EDGE_CACHE`,
`_TOPO_CACHE`) are keyed on the source tensor's address, strides, shape and version.  What makes that safe is that every
entry HOLDS its source: while the key is in the table the storage stays alive, so the address cannot be handed to
another tensor with other values.  These tests pin exactly that, by outcome, under a recycled address:

  * the allocator does recycle: a tensor made, dropped and made again comes back on its address (required: the test
    fails otherwise);
  * a first tensor is made, used and dropped in a frame that keeps no other reference; a second tensor of the same shape
    and dtype with OTHER values is made: with the memo as it is, it does not get the first one's address (the entry
    holds it) and its results equal those computed with the memo cleared;
  * control: the same scenario with the sources taken OUT of the memo's entries (what a memo that does not hold its
    source would be).  The second tensor then lands on the first one's address and the memo serves the first tensor's
    results for it.  So the scenario does reach the situation, and the assertions above would catch such a memo.

No defect is expected here.  That scenario needs an allocator that hands a freed block out again: the device's caching
allocator does, the host's does not (a freed host block is not returned to the next equal-sized request: measured, 0 of
64 requests), so it runs under the gpu mark.  Without a GPU the same memos are pinned on host tensors by what makes them
safe: the entry keeps the memory of its source alive after every other reference is gone, and (control) releases it once
the source is taken out of the entry."""
import gc
import weakref

import pytest
import torch

import handoffs as HO


def _faces(seed, n_faces, n_verts, dtype, device):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_verts, (n_faces, 3), generator=g).to("cpu").to(dtype).to(device)


def _first_use(make_first, use):
    """Make, use and drop the first tensor in this frame alone: the caller never holds it (its address is noted)."""
    first = make_first()
    HO.dropping(first)
    use(first)
    del first
    gc.collect()


def _scenario(make_first, make_second, use, clear, strip):
    """-> nothing; asserts the three points of the module's docstring.  use(t) -> tuple of result tensors (clones);
    clear() empties the memos; strip() replaces the source in every entry of the memos by None."""
    clear()
    # the allocator recycles
    probe = make_first()
    HO.dropping(probe)
    del probe
    again = HO.recycled(make_first)
    del again
    # the memo as it is
    _first_use(make_first, use)
    second = HO.pinned(make_second, attempts=4)[0]
    got = use(second)
    clear()
    want = use(second)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    del second, got
    clear()
    gc.collect()
    # control: entries that do not hold their source
    _first_use(make_first, use)
    stale = use(make_first())                          # (what the memo holds: the first tensor's results)
    strip()
    gc.collect()
    second = HO.recycled(make_second, attempts=8)      # on the first one's address now, or the test fails
    served = use(second)
    clear()
    want = use(second)
    assert not all(torch.equal(a, b) for a, b in zip(stale, want))
    assert all(torch.equal(a, b) for a, b in zip(served, stale)), \
        "a memo without its sources did not serve the stale result: the scenario does not reach the memo"
    clear()


def _strip_pairs(*tables):
    def strip():
        for t in tables:
            for k, (src, val) in list(t.items()):
                t[k] = (None, val)
    return strip


def _holds_on_the_host(make_first, use, clear, strip):
    """Host tensors: the first tensor lives in a numpy array's memory, which a weak reference can watch."""
    clear()
    arr = make_first().numpy().copy()
    watch = weakref.ref(arr)
    first = torch.from_numpy(arr)
    del arr
    use(first)
    del first
    gc.collect()
    assert watch() is not None, "the memo's entry does not keep its source alive"
    strip()
    gc.collect()
    assert watch() is None          # (control: the entry was the only holder, so the assertion above can fail)
    clear()


def _run(device, make_first, make_second, use, clear, strip):
    if device.type == "cpu":
        _holds_on_the_host(make_first, use, clear, strip)
    else:
        _scenario(make_first, make_second, use, clear, strip)


def _expand_faces(device):
    from acfm_video_3d_reconstruction_amd import ops
    N, F, V = 3, 37, 20

    def use(f):
        out = ops.expand_faces(f, N)
        assert out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (N, F, 3)
        return (out.clone(),)
    _run(device, lambda: _faces(1, F, V, torch.int32, device), lambda: _faces(2, F, V, torch.int32, device), use,
         ops._FACES.clear, _strip_pairs(ops._FACES))


def _packed_tables(device):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim import structures as S
    N, F, V = 2, 41, 16
    verts = torch.zeros(N, V, 3, device=device)

    def use(faces):
        m = S.Meshes(verts=verts, faces=faces)
        return m.faces_packed().clone(), m.edges_packed().clone()

    def clear():
        S._FACES_PACKED_CACHE.clear()
        S._EDGE_CACHE.clear()
        S._TOPO_CACHE.clear()

    def padded(seed):
        return _faces(seed, N * F, V, torch.int32, "cpu").reshape(N, F, 3).to(device)
    _run(device, lambda: padded(3), lambda: padded(4), use, clear,
         _strip_pairs(S._FACES_PACKED_CACHE, S._EDGE_CACHE, S._TOPO_CACHE))


def _list_topology(device):
    """A Meshes built from LISTS of faces tensors (how template_fit.fit_verts_to_mesh builds its meshes): the topology
    table is keyed on every tensor of the list."""
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim import structures as S
    F, V = 29, 12
    verts = [torch.zeros(V, 3, device=device)]

    def use(faces):
        m = S.Meshes(verts=verts, faces=[faces])
        return (m.edges_packed().clone(),)
    _run(device, lambda: _faces(5, F, V, torch.int64, device), lambda: _faces(6, F, V, torch.int64, device), use,
         S._TOPO_CACHE.clear, _strip_pairs(S._TOPO_CACHE))


BODIES = {"expand_faces_int32": _expand_faces, "meshes_packed_tables_padded": _packed_tables,
          "meshes_list_topology": _list_topology}


@pytest.mark.parametrize("which", sorted(BODIES))
def test_memo_entries_hold_their_sources(which):
    BODIES[which](torch.device("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(BODIES))
def test_memo_entries_hold_their_sources_on_the_device(which):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    BODIES[which](torch.device("cuda:0"))
