"""CPU: _lib.marshal, the one place a tensor becomes an address of the C ABI.  It is given real entries of
_lib.SIGNATURES, a torch.device and arguments; it needs neither the shared library nor a GPU."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

from acfm_video_3d_reconstruction_amd import _lib

CPU = torch.device("cpu")


def _marshal(name, args, device=CPU):
    return _lib.marshal(name, _lib.pointer_kinds(_lib.SIGNATURES[name][1]), device, args)


def _bds(**over):
    """Arguments of acfm_bds_loss (all but the stream) by the header's names: float* verts_xy, bds; uint8_t* vis;
    int32_t* sel; six ints; float* loss; int32_t* argmin; uint32_t* tickets; float* partials; size_t."""
    f, i32 = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    a = dict(verts_xy=f, bds=f, vis=torch.zeros(4, dtype=torch.uint8), sel=i32, N=1, V=2, P=2, ref_batch=1, rows=0, S=0,
             loss=f, argmin=i32, tickets=i32, partials=f, partial_floats=4)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values())


def _sil(**over):
    """Arguments of acfm_sil_forward: float* verts; int64_t* faces; float* cams; six ints; three floats; void* mask,
    pix_to_face; uint64_t* kth; uint8_t* vis; void* ws; size_t; tuning; extras."""
    f, i64 = torch.zeros(4), torch.zeros(4, dtype=torch.int64)
    a = dict(verts=f, faces=i64, cams=f, N=1, V=1, F=1, H=2, K=2, k_out=1, blur=0.0, sigma=1e-4, offset_z=0.0, mask=f,
             pix_to_face=i64, kth=i64, vis=torch.zeros(4, dtype=torch.uint8), ws=torch.zeros(8, dtype=torch.uint8),
             ws_bytes=8, tuning=None, extras=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values())


def _refused(exc, name, position, args, device=CPU):
    with pytest.raises(exc) as e:
        _marshal(name, args, device)
    assert name in str(e.value) and "parameter %d" % position in str(e.value), str(e.value)
    return str(e.value)


def test_the_table_names_the_kinds_these_tests_rely_on():
    """(position, label) of every pointer in front of the stream, and the parameter count with it."""
    count, pointers = _lib.pointer_kinds(_lib.SIGNATURES["acfm_bds_loss"][1])
    assert count == 16 and [p[:2] for p in pointers] == [
        (0, "float*"), (1, "float*"), (2, "int8*"), (3, "int32*"), (10, "float*"), (11, "int32*"), (12, "int32*"),
        (13, "float*")]
    count, pointers = _lib.pointer_kinds(_lib.SIGNATURES["acfm_sil_forward"][1])
    assert count == 21 and [p[:2] for p in pointers] == [
        (0, "float*"), (1, "int64*"), (2, "float*"), (12, "void*"), (13, "void*"), (14, "int64*"), (15, "int8*"),
        (16, "void*"), (18, "void*"), (19, "void*")]
    assert _lib.pointer_kinds(_lib.SIGNATURES["acfm_version"][1]) == (0, ())


def test_int32_where_int64_is_declared_is_refused():
    msg = _refused(TypeError, "acfm_sil_forward", 1, _sil(faces=torch.zeros(4, dtype=torch.int32)))
    assert "int64*" in msg and "torch.int32" in msg


def test_float64_where_float_is_declared_is_refused():
    msg = _refused(TypeError, "acfm_bds_loss", 0, _bds(verts_xy=torch.zeros(4, dtype=torch.float64)))
    assert "float*" in msg and "torch.float64" in msg


def test_float16_where_float_is_declared_is_refused():
    msg = _refused(TypeError, "acfm_bds_loss", 10, _bds(loss=torch.zeros(4, dtype=torch.float16)))
    assert "float*" in msg and "torch.float16" in msg


def test_float_where_an_integer_of_the_same_size_is_declared_is_refused():
    _refused(TypeError, "acfm_bds_loss", 12, _bds(tickets=torch.zeros(4)))


def test_a_transposed_tensor_is_refused():
    t = torch.zeros(4, 4).t()
    assert t.data_ptr() == t.t().data_ptr()           # what went through unseen
    msg = _refused(ValueError, "acfm_bds_loss", 1, _bds(bds=t))
    assert "contiguous" in msg


def test_a_strided_slice_is_refused_also_where_any_element_type_will_do():
    msg = _refused(ValueError, "acfm_sil_forward", 12, _sil(mask=torch.zeros(4, 4)[:, ::2]))
    assert "contiguous" in msg


def test_a_tensor_on_another_device_than_the_launch_is_refused():
    msg = _refused(ValueError, "acfm_sil_forward", 0, _sil(), device=torch.device("cuda", 0))
    assert "cpu" in msg and "cuda:0" in msg
    _refused(ValueError, "acfm_sil_forward", 16, [None] * 16 + _sil()[16:], device=torch.device("cuda", 0))


def test_one_argument_too_many_and_one_too_few_are_refused():
    for args, got in ((_bds() + [None], 16), (_bds()[:-1], 14)):
        with pytest.raises(TypeError) as e:
            _marshal("acfm_bds_loss", args)
        assert "acfm_bds_loss" in str(e.value) and "16" in str(e.value) and "got %d" % got in str(e.value)


def test_an_unformed_lazy_grad_is_refused_and_stays_unformed():
    from acfm_video_3d_reconstruction_amd.ops.base import LazyGrad
    formed = []
    g = LazyGrad(torch.zeros(4), "mask_losses", (torch.zeros(4),), lambda: formed.append(1) or torch.ones(4))
    msg = _refused(ValueError, "acfm_bds_loss", 0, _bds(verts_xy=g))
    assert "LazyGrad" in msg and "storage" in msg
    assert not formed and not g.is_materialized


def test_an_unformed_lazy_pix_to_face_is_refused_and_stays_unformed():
    from acfm_video_3d_reconstruction_amd.ops.render import LazyPixToFace
    formed = []
    p = LazyPixToFace(torch.zeros((1, 2, 2, 1), dtype=torch.int64), 4, lambda: formed.append(1))
    _refused(ValueError, "acfm_sil_forward", 13, _sil(pix_to_face=p))
    assert not formed and not p.is_materialized


def test_what_is_accepted_becomes_the_address():
    f32 = torch.zeros(4)
    out = _marshal("acfm_bds_loss", _bds(verts_xy=f32))
    assert out[0] == f32.data_ptr() and out[4:10] == [1, 2, 2, 1, 0, 0] and out[14] == 4
    for mask in (torch.zeros(4, dtype=torch.float16), torch.zeros(4)):                       # void*
        assert _marshal("acfm_sil_forward", _sil(mask=mask))[12] == mask.data_ptr()
    kth = torch.zeros(4, dtype=torch.int64)                                                  # uint64_t*
    assert _marshal("acfm_sil_forward", _sil(kth=kth))[14] == kth.data_ptr()
    tk = torch.zeros(4, dtype=torch.int32)                                                   # uint32_t*
    assert _marshal("acfm_bds_loss", _bds(tickets=tk))[12] == tk.data_ptr()
    vis = torch.zeros(4, dtype=torch.bool)                                                   # uint8_t*
    assert _marshal("acfm_bds_loss", _bds(vis=vis))[2] == vis.data_ptr()
    counts = torch.zeros(4, dtype=torch.int32)                                               # int*
    out = _marshal("acfm_boundaries", [f32, 1, 2, 2, 4, f32, counts])
    assert out[6] == counts.data_ptr()


def test_none_stays_null_and_a_zero_element_tensor_passes():
    out = _marshal("acfm_bds_loss", _bds(sel=None, partials=torch.zeros(0)))
    assert out[3] is None and out[13] == 0
    ctypes.c_void_p.from_param(out[13])


def test_ctypes_values_pass_through_untouched():
    vp, arr, tune = ctypes.c_void_p(0x1000), (ctypes.c_float * 4)(), _lib.RasterTuning()
    ref = ctypes.byref(tune)
    out = _marshal("acfm_sil_forward", _sil(verts=vp, cams=arr, tuning=ref))
    assert out[0] is vp and out[2] is arr and out[18] is ref


def test_a_pending_term_is_marshalled_without_launching_its_job(monkeypatch):
    """A PendingTerm over a CPU tensor, built by hand: marshal reads its device, dtype, contiguity and address only."""
    from acfm_video_3d_reconstruction_amd.ops import pending
    storage = torch.zeros(4)

    class Job:
        done = False
        out = storage

        def flush(self):
            self.done = True
    job = Job()
    term = pending.PendingTerm(storage, job)
    assert _marshal("acfm_bds_loss", _bds(loss=term))[10] == storage.data_ptr()
    assert not job.done and term.is_pending
    _refused(TypeError, "acfm_sil_forward", 1, _sil(faces=term))      # refusing one does not launch it either
    assert not job.done
    term + 1                                                          # (the hand-built job does flush on a real use)
    assert job.done


_STUB = """
static void* seen_stream;
static int calls;
int acfm_version(void) { return %d; }
int acfm_camera_mirror(const float* cams, int R, float* out, void* stream) {
  out[0] = cams[0] + (float)R; seen_stream = stream; ++calls; return 0;
}
void* stub_seen_stream(void) { return seen_stream; }
int stub_calls(void) { return calls; }
"""

_DRIVER = """
import contextlib, ctypes, torch
from acfm_video_3d_reconstruction_amd import _lib
_lib.cur_stream = lambda device: ctypes.c_void_p(0x5EED)      # no GPU here: a stand-in stream,
torch.cuda.device = lambda device: contextlib.nullcontext()   # and no device to switch to
cpu = torch.device("cpu")
cams, out = torch.full((7,), 2.0), torch.zeros(7)
_lib.call("acfm_camera_mirror", cpu, cams, 3, out)
h = _lib.lib()
h.stub_seen_stream.restype = ctypes.c_void_p
assert out[0].item() == 5.0 and h.stub_seen_stream() == 0x5EED and h.stub_calls() == 1
for args in ((cams, 3, out, _lib.ptr(out)), (cams, 3)):       # a stream of the caller's own in front; one short
    try:
        _lib.call("acfm_camera_mirror", cpu, *args)
    except TypeError as e:
        assert "acfm_camera_mirror" in str(e) and "takes 4" in str(e) and "got %d" % len(args) in str(e), e
    else:
        raise SystemExit("%d arguments went through" % len(args))
assert h.stub_calls() == 1
h.acfm_camera_mirror(_lib.ptr(cams), 3, _lib.ptr(out), None, None)   # what ctypes itself lets through: one too many
assert h.stub_calls() == 2
print("stub ok")
"""


def test_call_appends_exactly_one_stream_and_counts_it(tmp_path):
    """End to end against a stand-in library built with cc: every symbol of the table, acfm_camera_mirror recording the
    stream it was given.  call() passes the tensors' addresses and one stream behind them; an argument more or less is
    refused before the library is reached -- which ctypes alone does not do."""
    cc = next(c for c in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang")) if c)
    src, so = tmp_path / "stub.c", tmp_path / "libacfm_stub.so"
    rest = [n for n in _lib.SIGNATURES if n not in ("acfm_version", "acfm_camera_mirror")]
    src.write_text(_STUB % _lib.ABI_VERSION + "".join("int %s(void) { return 0; }\n" % n for n in rest))
    subprocess.check_call([cc, "-shared", "-fPIC", "-o", str(so), str(src)])
    r = subprocess.run([sys.executable, "-c", _DRIVER], cwd=ROOT, env=dict(os.environ, ACFM_LIB=str(so)),
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("stub ok"), r.stdout + r.stderr
