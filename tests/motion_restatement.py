"""Exact restatements and first-order forward error bounds for flexam_amd.motion (csrc/motion.hip), shared by the tests, the fixture
generator (tools/make_golden_motion.py) and tools/motion_bench.py.

Float32 chain (apply_motion, w2s_moge, convert_moge_to_delta_format, moge_tracks): the restatement runs in float64 torch (CPU or GPU)
on the float32 inputs; every function returns (value, bound) where `bound` B is the first-order forward bound of a float32 evaluation
in ANY summation order.  With u = 2^-24 and gamma_n = n u / (1 - n u):
  n-term product  y = sum_k a_k x_k:     B_y = gamma_n sum |a_k| |x_k| + sum |a_k| B_x_k
  quotient        q = a / b:             B_q = u |q| + B_a / |b| + |q| B_b / |b|
  product with an exact factor s:        B = |s| B_x + u |s x|
The tests assert |computed - exact| <= 2 B (the factor 2 covers the second-order terms) for the HIP results AND for the reference's
own float32 results in the fixtures.

Object-motion matrices are made on the host in float32 from a float32 centre: A = translate(c) . m . translate(-c), column
fl(fl(m (-c)) + c) (a 4-term product and one addition; two more roundings when MoGe's x / y translation is divided by W / H).  The
restatement uses the EXACT centre c* (float64 mean of the selected points) and the float32 matrix m as data; the matrix actually used
may differ from it by |I - R| |c - c*| + gamma_7 (|R| |c| + |t| + |c|) in its translation column, which enters the bound.

Float64 chain (s2w_vggt, w2s_vggt): the restatement runs in numpy longdouble (64-bit significand on x86), u = 2^-53."""
import numpy as np
import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(n, u=U32):
    return n * u / (1 - n * u)


def _mm(a, x):
    """[T, 3, 3] (or [3, 3]) times [T, N, 3] points."""
    return torch.einsum("...ij,tnj->tni", a, x) if a.dim() == 2 else torch.einsum("tij,tnj->tni", a, x)


def affine32(A, p, bp, col_err=None, sel=None):
    """p' = A[:, :, :3] p + A[:, :, 3] for A [T, 3, 4], p / bp [T, N, 3] (value, bound), float64 tensors.  col_err [T, 3]: bound on the
    deviation of the translation column actually used.  sel [N] bool: only these points move."""
    R, t = A[:, :, :3], A[:, :, 3]
    val = _mm(R, p) + t[:, None, :]
    b = gamma(4) * (_mm(R.abs(), p.abs()) + t.abs()[:, None, :]) + _mm(R.abs(), bp)
    if col_err is not None:
        b = b + col_err[:, None, :]
    if sel is not None:
        val = torch.where(sel[None, :, None], val, p)
        b = torch.where(sel[None, :, None], b, bp)
    return val, b


def project32(P, K, p, bp):
    """w2s_moge: c = P (p, 1); h = K c; (h_x / h_z, h_y / h_z, c_z)."""
    c, bc = affine32(P, p, bp)
    Kt = K.expand(P.shape[0], 3, 3) if K.dim() == 2 else K
    h = _mm(Kt, c)
    bh = gamma(3) * _mm(Kt.abs(), c.abs()) + _mm(Kt.abs(), bc)
    q = h[..., :2] / h[..., 2:3]
    bq = U32 * q.abs() + bh[..., :2] / h[..., 2:3].abs() + q.abs() * bh[..., 2:3] / h[..., 2:3].abs()
    return torch.cat([q, c[..., 2:3]], -1), torch.cat([bq, bc[..., 2:3]], -1)


def scale32(p, bp, width, height):
    s = torch.tensor([float(width), float(height), 1.0], dtype=p.dtype, device=p.device)
    val = p * s
    return val, bp * s + U32 * val.abs() * torch.tensor([1.0, 1.0, 0.0], dtype=p.dtype, device=p.device)


def exact_center(points0, sel):
    """float64 mean of the selected rows of points0 [N, 3] (float32 data)."""
    return points0.double()[sel].mean(dim=0)


def exact_object_motion(m, c_star, c_used, moge_hw=None):
    """m [T, 4, 4] float32 motion about the origin (rotation or translation), c_star exact centre, c_used the float32 centre the host
    used -> (A [T, 3, 4] float64 = translate(c*) m translate(-c*), col_err [T, 3])."""
    m = m.double()
    R, t = m[:, :3, :3], m[:, :3, 3]
    col = c_star[None, :] - torch.einsum("tij,j->ti", R, c_star) + t
    eye = torch.eye(3, dtype=torch.float64, device=m.device)
    dc = (c_used.double() - c_star).abs()
    err = torch.einsum("tij,j->ti", (eye[None] - R).abs(), dc)
    err = err + gamma(7) * (torch.einsum("tij,j->ti", R.abs(), c_used.double().abs()) + t.abs() + c_used.double().abs()[None, :])
    if moge_hw is not None:
        d = torch.tensor([float(moge_hw[1]), float(moge_hw[0]), 1.0], dtype=torch.float64, device=m.device)
        col, err = col / d, err / d
    return torch.cat([R, col[:, :, None]], dim=2), err


def motion_about_origin(motion_type, distance, num_frames):
    """The float32 m of object_motion_matrices: what it returns for a zero centre (translate(0) is exact)."""
    from flexam_amd.motion import object_motion_matrices
    return object_motion_matrices(torch.zeros(3), motion_type, distance, num_frames)


def close32(got, exact, bound):
    """|got - exact| <= 2 B elementwise, NaN exactly where the restatement has NaN.  Returns (ok, worst ratio)."""
    got = got.double()
    nan = torch.isnan(exact)
    if not torch.equal(torch.isnan(got), nan):
        return False, float("inf")
    same = nan | (got == exact)                                  # equal values pass whatever the bound (a division by an exact 0: +-inf both sides)
    ratio = torch.where(same, torch.zeros_like(exact), (got - exact).abs() / (2 * bound).clamp_min(1e-300))
    if bool(torch.isnan(ratio).any()):
        return False, float("nan")
    return bool((ratio <= 1).all()), float(ratio.max()) if ratio.numel() else 0.0


# ----------------------------------------------------------------------------- float64 chain, restated in longdouble
LD = np.longdouble


def _mm_ld(a, x):
    return np.einsum("tij,tnj->tni", a, x)


def unproject64(points, kinv, rinv, tvec):
    """s2w_vggt in longdouble: (world [T, N, 3], bound for a float64 evaluation, valid [T, N])."""
    p = np.asarray(points).astype(LD)
    kinv, rinv, tvec = (np.asarray(a).astype(LD) for a in (kinv, rinv, tvec))
    uv1 = np.concatenate([p[..., :2], np.ones(p.shape[:2] + (1,), LD)], -1)
    z = p[..., 2:3]
    cam = _mm_ld(kinv, uv1) * z
    bcam = (gamma(3, U64) * _mm_ld(np.abs(kinv), np.abs(uv1)) * np.abs(z) + U64 * np.abs(cam))
    d = cam - tvec[:, None, :]
    bd = bcam + U64 * np.abs(d)
    w = _mm_ld(rinv, d)
    bw = gamma(3, U64) * _mm_ld(np.abs(rinv), np.abs(d)) + _mm_ld(np.abs(rinv), bd)
    valid = p[..., 2] > 0
    return np.where(valid[..., None], w, 0), np.where(valid[..., None], bw, 0), valid


def project64(points, pose, intr):
    """w2s_vggt in longdouble: ((u, v, depth) [T, N, 3], bound, valid [T, N], depth before the validity test)."""
    p = np.asarray(points).astype(LD)
    pose, intr = np.asarray(pose).astype(LD), np.asarray(intr).astype(LD)
    R, t = pose[:, :3, :3], pose[:, :3, 3]
    c = _mm_ld(R, p) + t[:, None, :]
    bc = gamma(4, U64) * (_mm_ld(np.abs(R), np.abs(p)) + np.abs(t)[:, None, :])
    den = c[..., 2:3] + LD(1e-10)
    bden = bc[..., 2:3] + U64 * np.abs(den)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = c / den
        bn = U64 * np.abs(n) + bc / np.abs(den) + np.abs(n) * bden / np.abs(den)
    uv = _mm_ld(intr, n)
    buv = gamma(3, U64) * _mm_ld(np.abs(intr), np.abs(n)) + _mm_ld(np.abs(intr), bn)
    valid = c[..., 2] > 0
    out = np.concatenate([uv[..., :2], c[..., 2:3]], -1)
    bound = np.concatenate([buv[..., :2], bc[..., 2:3]], -1)
    return np.where(valid[..., None], out, 0), np.where(valid[..., None], bound, 0), valid, c[..., 2]


def close64(got, exact, bound, extra=None):
    """|got - exact| <= 2 B (+ extra) elementwise in longdouble."""
    err = np.abs(np.asarray(got).astype(LD) - exact)
    lim = 2 * bound + (0 if extra is None else extra)
    return bool((err <= lim).all()), float(np.max(err / np.maximum(lim, np.finfo(LD).tiny))) if err.size else 0.0


def vggt_host_matrices(extrinsics, intrinsics, poses=None, override_extrinsics=True, T=None):
    """The O(T) host half of s2w_vggt / w2s_vggt with the reference's numpy calls: (kinv, rinv, tvec, pose [T, 3, 4], intr) as float64."""
    ext = extrinsics.numpy() if isinstance(extrinsics, torch.Tensor) else np.asarray(extrinsics)
    itr = intrinsics.numpy() if isinstance(intrinsics, torch.Tensor) else np.asarray(intrinsics)
    ext, itr = (ext[0] if ext.ndim == 4 else ext), (itr[0] if itr.ndim == 4 else itr)
    T = ext.shape[0] if T is None else T
    kinv = np.stack([np.linalg.inv(itr[i]) for i in range(T)]).astype(np.float64)
    rinv = np.stack([np.linalg.inv(ext[i, :, :3]) for i in range(T)]).astype(np.float64)
    tvec = ext[:T, :, 3].astype(np.float64)
    if poses is None:
        first = np.eye(4)
        first[:3, :] = ext[0]
        cam = np.tile(first[None], (T, 1, 1))
    else:
        given = poses.numpy() if isinstance(poses, torch.Tensor) else np.asarray(poses)
        cam = given.copy()
        cam[:, :3, 3] = given[:, :3, 3] / 5.0
        if not override_extrinsics:
            for i in range(T):
                e = np.eye(4)
                e[:3, :] = ext[i]
                cam[i] = np.matmul(cam[i], e)
    return kinv, rinv, tvec, cam[:T, :3, :].astype(np.float64), itr[:T].astype(np.float64)
