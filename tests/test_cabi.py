"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/acfm_hip.h declares; the Python layer refuses to run without a GPU (no fallback)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def _header():
    """include/acfm_hip.h without its comments."""
    txt = open(os.path.join(ROOT, "include", "acfm_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _declared_symbols():
    return sorted(set(re.findall(r"\b(acfm_[a-z0-9_]+)\s*\(", _header())))


_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
# what a device pointer points to, as _lib.SIGNATURES names it: element size and float-versus-integer, not signedness
_ELEMENTS = {"float": "float*", "double": "double*", "uint8_t": "int8*", "int": "int32*", "int32_t": "int32*",
             "uint32_t": "int32*", "int64_t": "int64*", "uint64_t": "int64*"}


def _kind(param):
    """A parameter `type name` of the header as the table holds it: int / float / size_t are their ctypes classes (a
    scalar type outside these is a KeyError: extend the test with the ABI); a pointer to float, double or a 1-, 4- or
    8-byte integer on the device is its element kind; void*, a mirrored structure, a pointer table and a host
    out-parameter (`*_host`, size_t*) are c_void_p; a pointer to anything else is a KeyError as well."""
    base, name = param.rsplit(" ", 1)
    if "*" not in param:
        return _SCALARS[base]
    base = base.replace("const ", "").rstrip("* ")
    if param.count("*") > 1 or name.endswith("_host") or base in ("void", "size_t") or base.lower().startswith("acfm"):
        return ctypes.c_void_p
    return _ELEMENTS[base]


def _prototypes():
    """{name: (restype, [parameter kinds])} of every `type name(args);` of the header (see _kind)."""
    out = {}
    for ret, name, args in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*(acfm_\w+)\s*\(([^()]*)\)\s*;", _header(), flags=re.M):
        params = [" ".join(a.split()) for a in args.split(",")]
        if params == ["void"]:
            params = []
        kinds = [_kind(p) for p in params]
        assert name not in out, "%s is declared twice" % name
        out[name] = (_RETURNS[" ".join(ret.split())], kinds)
    return out


def _struct_fields(name):
    """Field names, in order, of `typedef struct [tag] { ... } name;` (several fields per statement are split)."""
    body = re.search(r"typedef\s+struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*%s\s*;" % name, _header()).group(1)
    pieces = [p.strip() for p in re.split(r"[;,]", body)]
    return [re.search(r"(\w+)\s*(?:\[\d+\])?$", p).group(1) for p in pieces if p]


def _defines():
    """{NAME: value} of the header's integer #defines and enumerators."""
    txt = _header()
    out = {k: int(v, 0) for k, v in re.findall(r"^#define\s+(ACFM_\w+)\s+(-?\w+)\s*$", txt, flags=re.M)}
    for body in re.findall(r"enum\s*\{([^{}]*)\}", txt):
        out.update({k: int(v, 0) for k, v in re.findall(r"(ACFM_\w+)\s*=\s*(-?\w+)", body)})
    return out


def test_signature_table_matches_the_header_by_type():
    """SIGNATURES[name] == the header's prototype: return type and every parameter's class -- for a device pointer the
    element kind it points to -- in order and in number (the names-only comparison below cannot see an argument added
    to or dropped from one side)."""
    from acfm_video_3d_reconstruction_amd import _lib
    protos = _prototypes()
    assert set(protos) == set(_declared_symbols()), "a prototype the pattern does not parse"
    assert set(protos) == set(_lib.SIGNATURES)
    short = lambda sig: "%s(%s)" % (sig[0].__name__, ", ".join(getattr(k, "__name__", k) for k in sig[1]))
    bad = ["%s: header %d parameters %s, table %d parameters %s" % (n, len(h[1]), short(h), len(t[1]), short(t))
           for n, h in sorted(protos.items()) for t in [_lib.SIGNATURES[n]] if h != (t[0], list(t[1]))]
    assert not bad, "\n".join(bad)


def test_mirrored_structures_match_the_header():
    from acfm_video_3d_reconstruction_amd import _lib
    pairs = [(_lib.RasterTuning, "AcfmRasterTuning"), (_lib.SilExtras, "AcfmSilExtras"),
             (_lib.BlendParams, "AcfmBlendParams"), (_lib.StepMaskJob, "acfm_step_mask_job"),
             (_lib.StepTexJob, "acfm_step_tex_job"), (_lib.StepBdsJob, "acfm_step_bds_job"),
             (_lib.StepTotalJob, "acfm_step_total_job")]
    for cls, name in pairs:
        assert [f[0] for f in cls._fields_] == _struct_fields(name), name


def test_mirrored_constants_match_the_header():
    from acfm_video_3d_reconstruction_amd import _lib, ops
    from acfm_video_3d_reconstruction_amd.ops import base
    d = _defines()
    assert _lib.PROF_NKERNELS == d["ACFM_PROF_NKERNELS"]
    assert set(_lib._ERR) == {d["ACFM_E_BADARG"], d["ACFM_E_LAUNCH"], d["ACFM_E_WORKSPACE"]} and d["ACFM_OK"] == 0
    assert [_lib._ERR[d[k]].split()[0] for k in ("ACFM_E_BADARG", "ACFM_E_LAUNCH", "ACFM_E_WORKSPACE")] == \
        ["ACFM_E_BADARG", "ACFM_E_LAUNCH", "ACFM_E_WORKSPACE"]
    assert _lib.raster_tuning(deterministic=True).t.flags == d["ACFM_DETERMINISTIC"] == 1
    assert _lib.with_f16(None, True).flags == d["ACFM_STORE_F16"] == 2
    assert _lib.with_cover(None, True).flags == d["ACFM_RECORD_COVER"] == 4
    assert ops.SOLVE_INFO_HANDOFF == d["ACFM_SOLVE_INFO_HANDOFF"]
    assert ops.GEODESIC_MAX_STEINER == d["ACFM_GEODESIC_MAX_STEINER"]
    assert ops.GEODESIC_LDS_MAX == d["ACFM_GEODESIC_LDS_MAX"]
    assert (base._LOSS_MASK, base._LOSS_TEX_MSE, base._LOSS_BDS) == \
        (d["ACFM_LOSS_MASK"], d["ACFM_LOSS_TEX_MSE"], d["ACFM_LOSS_BDS"]) == (0, 1, 2)


def test_a_library_of_another_version_is_refused_at_load(tmp_path):
    """ACFM_LIB pointing at a build that reports another acfm_version(): _lib.lib() raises before it binds any other
    symbol (the 2.x entry points keep 1.x names with other argument lists), naming the file, both versions and the
    rebuild command.  The stand-in exports acfm_version alone, so reaching any other symbol would be an AttributeError."""
    import shutil
    import subprocess
    import sys
    from acfm_video_3d_reconstruction_amd import _lib
    cc = next(c for c in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang")) if c)
    src, so = tmp_path / "stale.c", tmp_path / "libacfm_stale.so"
    src.write_text("int acfm_version(void) { return 1001; }\n")
    subprocess.check_call([cc, "-shared", "-fPIC", "-o", str(so), str(src)])
    r = subprocess.run([sys.executable, "-c", "from acfm_video_3d_reconstruction_amd import _lib; _lib.lib()"],
                       cwd=ROOT, env=dict(os.environ, ACFM_LIB=str(so)), capture_output=True, text=True)
    assert r.returncode != 0
    assert _lib.ABI_VERSION == 2000
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith("RuntimeError:") and str(so) in last and "1001" in last and "2000" in last, r.stderr
    assert "make -C" in last and _lib.CSRC in last, r.stderr


def test_library_exports_every_declared_symbol():
    from acfm_video_3d_reconstruction_amd import _lib
    _lib.build()
    assert os.path.exists(_lib.SO_PATH)
    raw = ctypes.CDLL(_lib.SO_PATH)
    syms = _declared_symbols()
    assert len(syms) >= 15
    for name in syms:
        assert hasattr(raw, name), "libacfm_hip.so does not export %s" % name
    assert set(syms) == set(_lib.SIGNATURES), "ctypes signature table out of sync with the header"
    h = _lib.lib()
    assert h.acfm_arch() == b"gfx950"
    assert h.acfm_raster_workspace_bytes(64, 642, 1280, 256) > 0
    assert h.acfm_raster_workspace_bytes(0, 642, 1280, 256) == 0


def test_library_exports_nothing_undeclared():
    """No hidden knobs: every acfm_* symbol the shipping library exports is declared in the public
    header (the acfm_debug_* diagnostics exist only in the DIAG build, tuning is per call)."""
    import subprocess
    from acfm_video_3d_reconstruction_amd import _lib
    _lib.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("acfm_")}
    assert exported == set(_declared_symbols()), sorted(exported ^ set(_declared_symbols()))
    assert not any("debug" in s for s in exported)


def test_deform_apply_backward_refuses_a_grid_past_int_range():
    """k_deform_bwd_dm indexes its ceil(Kh/16) ceil(3N/16) tiles with ints: past 2^31 - 1 workgroups the entry point
    returns ACFM_E_BADARG (1) before anything is launched or read (the pointers here are never dereferenced)."""
    from acfm_video_3d_reconstruction_amd import _lib
    _lib.build()
    fake = ctypes.c_void_p(0x1000)
    args = (fake, fake, fake, 1000000, 1, 200000)              # 12500 x 187500 tiles = 2.34e9
    assert _lib.lib().acfm_deform_apply_backward(*args, fake, fake, None, None) == 1
    assert _lib.lib().acfm_deform_apply_backward(*args, fake, None, None, None) == 1
    assert _lib.lib().acfm_deform_apply_backward(*args, None, fake, None, None) == 1


def test_no_cpu_fallback():
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.nnutils.nmr import NeuralRenderer
    v = torch.zeros(1, 4, 3)
    f = torch.zeros(1, 2, 3, dtype=torch.int64)
    c = torch.zeros(1, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NeuralRenderer(32)(v, f, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.project(v, c)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under the product package may reference it."""
    pkg = os.path.join(ROOT, "acfm_video_3d_reconstruction_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".inc", ".cpp")):
                src = open(os.path.join(dp, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), fn
                assert "libacfm_oracle" not in src, fn
                assert '#include "../../oracle' not in src and "oracle/acfm_oracle" not in src.replace(
                    "oracle/acfm_oracle.c is the bit-level spec", ""), fn


def test_cover_flag_policy_and_tuning_helpers():
    """ACFM_RECORD_COVER is decided on the host (ops._cover_tuning / _cover_taken): off until a texture render has taken
    a silhouette render's workspace over, off again once a recorded plane went unread; raster_tuning(record_cover=...)
    forces it; the helpers never mutate the caller's structure and keep the other flag bits."""
    import torch
    from acfm_video_3d_reconstruction_amd import _lib, ops
    dev = torch.device("cpu")          # the policy is pure host logic: any hashable device key
    ops._COVER.pop(dev, None)
    flag = lambda t: bool(t is not None and t.flags & 4)
    assert not flag(ops._cover_tuning(dev, None))                 # nothing seen yet
    assert ops._cover_taken(dev, None) == 1                       # taken over, but no plane was recorded
    t = ops._cover_tuning(dev, None)
    assert flag(t) and ops._cover_taken(dev, t) == 2              # recorded and read
    assert flag(ops._cover_tuning(dev, None))
    assert not flag(ops._cover_tuning(dev, None))                 # the previous plane was never read
    assert not flag(ops._cover_tuning(dev, None))
    # forced either way, whatever the state; the deterministic / f16 bits survive
    with _lib.raster_tuning(deterministic=True, record_cover=True) as rt:
        t = ops._cover_tuning(dev, rt.t)
        assert t.flags == 5 and rt.t.flags == 1
        t16 = _lib.with_f16(t, True)
        assert t16.flags == 7 and t.flags == 5
    with _lib.raster_tuning(record_cover=False) as rt:
        ops._COVER[dev] = {"on": True, "pending": False}
        assert not flag(ops._cover_tuning(dev, rt.t))
    assert _lib.with_cover(None, False) is None and _lib.with_cover(None, True).flags == 4
    ops._COVER.pop(dev, None)
