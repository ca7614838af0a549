"""Half storage (storage="f16", AcfmRasterTuning.flags bit 1) as an exact model on the host: numpy only, no GPU.

csrc/acfm_raster.h:104-107 defines it: "Only what is STORED changes: every accept / reject decision, depth, blend
factor and loss sum is computed in fp32 exactly as in the fp32 build".  The five rules below say where a stored (and so
rounded) value is read back and where the unrounded fp32 value is used; each function restates the kernel lines its
docstring cites.  With them the expected answers of the half build follow from quantities of the fp32 build, which the
suite pins to the oracle, and the two builds are compared at the fp32 bars.

  1. stored mask / silhouette / image = h(fp32 value); ids are the fp32 ids, as an int32 plane
  2. fused silhouette losses: sums over the UNROUNDED mask and the half references
  3. silhouette backward: reads the half mask, so it is the fp32 backward of the upstream gradient times
     ratio(m32, m_h)
  4. fused texture MSE forward: the unrounded image of the half atlas against the half references
  5. fused texture MSE backward: reads the stored half image

What a GPU comparison at the fp32 bars can tell apart (tests/test_gpu_half_storage.py): the two readings of the mask
in rule 3 lie 160 to 350 bars apart, and summing the rounded mask in rule 2 is 2 bars out.  Rules 4 and 5 differ
only in whether the image is rounded first, and a covered pixel's value is wnum c / (wnum + 1e-10) with wnum >= 0.5
(csrc/acfm_raster.hip:857-880): the half texel c to within an ulp of float32.  There "stored" and "unrounded" are 2^-24
apart, below any bar; the rules still say which one the kernel reads.

A sixth rule is autograd's, not a kernel's: the gradient of a float16 output is handed to its operator in float16, so an
upstream gradient g of the half mask arrives as h(g).

Batches of references and atlases: mesh n reads reference / atlas n % B (ops.base._ref_batch)."""
import numpy as np

f32 = np.float32


def h(x):
    """float32 -> IEEE half -> float32, round to nearest even, subnormals kept: what `(half_t)v` of st_real
    (csrc/acfm_raster.h:114-116) followed by `(float)` of ld_real (:109-111) does, and torch's .half().float()."""
    return np.asarray(x, f32).astype(np.float16).astype(f32)


def _per_mesh(ref, N):
    """[B,...] -> [N,...]: mesh n reads reference n % B."""
    ref = np.asarray(ref)
    return ref[np.arange(N) % ref.shape[0]]


# ------------------------------------------------------------------------------------------------ rule 1: what is stored
def stored(v32):
    """The half tensor a kernel leaves for the fp32 value v32 (mask: csrc/acfm_raster.hip:1049; image and silhouette:
    :846-847, :881-882; all through st_real) -> float16 array.  +0 stays +0: an empty pixel holds the bits 0x0000."""
    return np.asarray(v32, f32).astype(np.float16)


def stored_ids(p2f):
    """The nearest-face plane of half storage: st_face (csrc/acfm_raster.h:124-127) narrows the same id to int32;
    [N,H,H,k] int64 (slot 0 is the nearest face) -> [N,H,H,1] int32."""
    return np.asarray(p2f)[..., :1].astype(np.int32)


# ------------------------------------------------------------------------------------------------ rule 2: fused silhouette losses
def fused_sil_losses(m32, g_h, e_h):
    """csrc/acfm_raster.hip:1039-1064 and csrc/acfm_raster_api.hip:20-75.  The block sums take lmask = 1 - alpha, the
    fp32 value BEFORE st_real rounds it (:1049-1051), and the references through ld_real from their half tensors
    (:1042-1043; the finish kernel's sum of gt likewise, api:41, :48).  m32 [N,H,H] float32, g_h / e_h [B,H,H]
    values of the half references -> [N,4] float64 = (mean|m - g|, sum m g, sum(m + g - m g), mean e m)."""
    m = np.asarray(m32, f32).astype(np.float64)
    N = m.shape[0]
    g = _per_mesh(np.asarray(g_h, f32), N).astype(np.float64).reshape(N, -1)
    e = _per_mesh(np.asarray(e_h, f32), N).astype(np.float64).reshape(N, -1)
    m = m.reshape(N, -1)
    return np.stack([np.abs(m - g).mean(1), (m * g).sum(1), (m + g - m * g).sum(1), (e * m).mean(1)], 1)


# ------------------------------------------------------------------------------------------------ rule 3: silhouette backward
def ratio(m32, m_h):
    """csrc/acfm_raster.hip:1329-1345: the backward reads m = ld_real(mask) -- the half mask in half storage -- and
    forms coef = -gm (1 - m) / sigma; nothing else of it depends on the storage (the K-th keys are fp32 decisions).
    So the half backward of an upstream gradient gm is the fp32 backward of gm * r with
    r = (1 - m_h) / (1 - m32), in float64 (both differences are exact there) and then float32; r = 0 where
    1 - m32 == 0 (then m_h == 1 too and both builds have coef = 0).  The branch `m != 0` (:1330) is the same in both
    storages: see zero_mask_agrees."""
    a = 1.0 - np.asarray(m32, f32).astype(np.float64)
    b = 1.0 - np.asarray(m_h, f32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a == 0, 0.0, b / a)
    return r.astype(f32)


def zero_mask_agrees(m32):
    """m_h == 0 exactly where m32 == 0 (-> bool): the mask is 1 - alpha with alpha a float32 in [0, 1], so it is 0 or at
    least 2^-24, and h(2^-24) is the smallest half subnormal, not 0."""
    m32 = np.asarray(m32, f32)
    return bool(((h(m32) == 0) == (m32 == 0)).all())


def fused_grad_mask(m_h, g_h, e_h, go):
    """csrc/acfm_raster.hip:1335-1343, in float32 and in the kernel's order of operations: inv = 1 / HW,
    g0 = go[0] inv, g3 = go[3] inv, gm = g0 sgn(m - g) + g1 g + g2 (1 - g) + g3 e, with m the HALF mask and g, e the half
    references.  (The compiler may contract the products into fused multiply-adds: an ulp of difference.)
    m_h [N,H,H], g_h / e_h [B,H,H], go [N,4] -> [N,H,H] float32.  The kernel forms it only where m != 0; elsewhere
    coef = 0 whatever gm is."""
    m = np.asarray(m_h, f32)
    N, H = m.shape[0], m.shape[1]
    g, e = _per_mesh(np.asarray(g_h, f32), N), _per_mesh(np.asarray(e_h, f32), N)
    go = np.asarray(go, f32)
    inv = f32(1.0) / f32(H * m.shape[2])
    g0, g1, g2, g3 = ((go[:, k] * inv if k in (0, 3) else go[:, k])[:, None, None] for k in range(4))
    gm = g0 * np.sign(m - g) + g1 * g + g2 * (f32(1.0) - g) + g3 * e
    assert gm.dtype == f32
    return gm


# ------------------------------------------------------------------------------------------------ rule 4: fused texture MSE forward
def tex_mse_loss(v32, ref_h, mk_h):
    """csrc/acfm_raster.hip:876-893 (finish: csrc/acfm_raster_api.hip:77-135).  The texel comes from the half atlas
    (ld_real, :876-877); the blended value vr / vg / vb enters the difference as computed, before st_real rounds it for
    the stored image (:881, :891); reference image and mask are read from their half tensors (:887-890).  v32 [N,3,H,H]:
    the fp32 render of the atlas ROUNDED TO HALF; ref_h [B,3,H,H], mk_h [B,H,H] -> [N] float64,
    mean over (3,H,W) of (v mk - ref mk)^2."""
    v = np.asarray(v32, f32).astype(np.float64)
    N = v.shape[0]
    ref = _per_mesh(np.asarray(ref_h, f32), N).astype(np.float64)
    mk = _per_mesh(np.asarray(mk_h, f32), N).astype(np.float64)[:, None]
    return ((v * mk - ref * mk) ** 2).reshape(N, -1).mean(1)


# ------------------------------------------------------------------------------------------------ rule 5: fused texture MSE backward
def tex_mse_grad(x_h, ref_h, mk_h, go):
    """csrc/acfm_raster_texgrad.hip:69-101, form TEXG_MSE_F16: image, reference and mask are all loaded from half
    tensors (ld_plane with h16 = 1, :72-75) -- the image is the STORED one, unlike the forward -- and the gradient of
    a pixel is g' = w (x mk - ref mk) mk with w = go[n] 2 / (3 HW) (:81-83, :99), float32 in that order.
    x_h [N,3,H,H] values of the stored half image, go [N] -> [N,3,H,H] float32.  Its scatter sum over the texel
    indices (scatter_texels) is the atlas gradient."""
    x = np.asarray(x_h, f32)
    N, H, W = x.shape[0], x.shape[2], x.shape[3]
    ref = _per_mesh(np.asarray(ref_h, f32), N)
    mk = _per_mesh(np.asarray(mk_h, f32), N)[:, None]
    w = (np.asarray(go, f32) * f32(2.0) / (f32(3.0) * f32(H * W)))[:, None, None, None]
    g = w * (x * mk - ref * mk) * mk
    assert g.dtype == f32
    return g


def shared_tidx(tidx, NA, texels_per_mesh):
    """Texel indices of a render with one atlas per mesh ([N,H,H], texel = (n F + f) R^2 + ..) -> the indices when the
    N meshes share NA atlases (mesh n samples atlas n % NA, csrc/acfm_raster.hip:856); -1 stays."""
    tidx = np.asarray(tidx)
    n = np.arange(tidx.shape[0])[:, None, None]
    return np.where(tidx >= 0, tidx + ((n % NA) - n) * texels_per_mesh, tidx).astype(tidx.dtype)


def scatter_texels(g, tidx, atlas_shape):
    """float64 sum of g [N,3,H,H] over the pixels of every texel (tidx [N,H,H], -1: none) -> atlas_shape float64:
    hypotheses that share an atlas add up; a texel no pixel samples stays exactly 0."""
    out = np.zeros((int(np.prod(atlas_shape[:-1])), 3), np.float64)
    t = np.asarray(tidx).reshape(-1)
    sel = t >= 0
    np.add.at(out, t[sel], np.asarray(g, np.float64).transpose(0, 2, 3, 1).reshape(-1, 3)[sel])
    return out.reshape(atlas_shape)
