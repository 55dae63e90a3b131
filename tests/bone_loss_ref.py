"""The fp64 NumPy statement of the bone-vector loss's rule in include/hupr.h (``ref_bone``), the bone tables, the fixed cases and the
sign margin of the bone-loss tests.  Not a test module: tests/test_bone_loss_cpu.py checks the reference itself (against torch's fp64
autograd and on hand-built planes), tests/test_bone_loss_gpu.py compares the kernels with it."""
import numpy as np

from test_coord_loss_cpu import make_case, make_weights, ref_position  # noqa: F401  (re-exported for the two test modules)

SKELETON0 = ((13, 12), (12, 11), (10, 9), (9, 8), (8, 6), (11, 8), (7, 6), (6, 0), (6, 3), (5, 4), (4, 3), (2, 1), (1, 0))
STRIDE = 4.0
A0, A1, G = 0.3, 0.7, 1.7
FACTOR = 50.0

# (B, K, H) -> the seed of make_case: (3, 14, 64) the model's shape, (1, 2, 128) 64 terms per thread, (2, 17, 5) the 4-byte loads,
# (20, 14, 8) B E = 260 > 256, the one-workgroup loop's second trip, (1, 2, 5) the smallest case.  With these seeds, snap 0 and 1,
# |d| >= 50 (bound_u + bound_v) on both axes of every bone of both heads (test_bone_loss_cpu.py asserts it).
CASES = {(3, 14, 64): 4, (1, 2, 128): 0, (2, 17, 5): 18, (20, 14, 8): 9, (1, 2, 5): 0}


def bones_for(K):
    """K = 14: the data set's skeleton, zero-based; any other K: the chain (j, j + 1)."""
    return SKELETON0 if K == 14 else tuple((j, j + 1) for j in range(K - 1))


def make_bone_weights(E):
    """Per-bone weights with a zero and non-unit values (one weight of 2.0 when E = 1)."""
    if E == 1:
        return np.array([2.0], dtype=np.float32)
    w = np.random.RandomState(3000 + E).uniform(0.5, 2.0, E).astype(np.float32)
    w[E // 3] = 0.0
    return w


def ref_bone(p1, p2, joints, stride, snap, bones, w=None, eps=1.0, a0=1.0, a1=1.0, g=1.0, calls=1):
    """The whole rule in fp64.  p1, p2: (B, K, H, H) arrays (taken as float64 exactly), joints (B, K, 2), bones E zero-based pairs,
    w None or E weights.  -> dict with resid (2, B, K, 2), inv_den (2, B, K), valid (B, K), bone_valid (B, E), bone_resid
    (2, B, E, 2), gcoef (2, B, K, 2), incident (K,) = the summed |w_e| of a joint's bones, loss3 = (a0 B_0 + a1 B_1, B_0, B_1), acc
    (3,) after ``calls`` calls, dp (2, B, K, H, H) by the stated backward rule for the gradient g of loss3[0], and bound (2, B, K, 2) =
    5e-6 (A + |r|) + 1e-7 with A = sum p |x - a| / den, the error allowed to an fp32 residual (tests/test_coord_loss_gpu.py)."""
    p = np.stack([np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)])
    _, B, K, H, _ = p.shape
    uv = np.asarray(bones, dtype=np.int64).reshape(-1, 2)
    u, v = uv[:, 0], uv[:, 1]
    E = len(uv)
    wv = np.ones(E) if w is None else np.asarray(w, dtype=np.float64)
    a, valid = ref_position(joints, stride, snap, H)
    y, x = np.mgrid[0:H, 0:H].astype(np.float64)
    a_ = np.where(valid[..., None], a, 0.0)
    off = np.stack([x[None, None] - a_[..., 0, None, None], y[None, None] - a_[..., 1, None, None]])       # (2 axes, B, K, H, H)
    v5, v4, v3 = valid[None, :, :, None, None], valid[None, :, :, None], valid[None]
    with np.errstate(invalid="ignore"):
        pv = np.where(v5, p, 0.0)                                                                            # an invalid joint's plane is not read
        den = pv.sum(axis=(-1, -2)) + eps
        N = np.stack([(pv * off[0][None]).sum(axis=(-1, -2)), (pv * off[1][None]).sum(axis=(-1, -2))], axis=-1)
        A = np.stack([(pv * np.abs(off[0])[None]).sum(axis=(-1, -2)), (pv * np.abs(off[1])[None]).sum(axis=(-1, -2))], axis=-1)
        r = np.where(v4, N / den[..., None], 0.0)
        A = np.where(v4, A / den[..., None], 0.0)
        inv_den = np.where(v3, 1.0 / den, 0.0)
        bone_valid = valid[:, u] & valid[:, v]                                                               # (B, E)
        d = np.where(bone_valid[None, :, :, None], r[:, :, v] - r[:, :, u], 0.0)                             # (2, B, E, 2)
        Bh = (wv[None, None, :, None] * np.abs(d)).sum(axis=(1, 2, 3)) / (2 * B * E)
        sg = np.where(bone_valid[None, :, :, None], wv[None, None, :, None] * np.sign(d), 0.0)               # sign(nan) = nan
        gcoef = np.zeros((2, B, K, 2))
        for e in range(E):                                                                                   # bone-index order
            gcoef[:, :, v[e]] += sg[:, :, e]
            gcoef[:, :, u[e]] -= sg[:, :, e]
        f = (g * np.array([a0, a1]))[:, None, None] * inv_den / (2 * B * E)
        dp = f[..., None, None] * (gcoef[..., 0, None, None] * (off[0][None] - r[..., 0, None, None]) +
                                   gcoef[..., 1, None, None] * (off[1][None] - r[..., 1, None, None]))
        zero = (f == 0) | ((gcoef[..., 0] == 0) & (gcoef[..., 1] == 0))
        dp = np.where(zero[..., None, None], 0.0, dp)
        bound = 5e-6 * (A + np.abs(r)) + 1e-7
    incident = np.zeros(K)
    np.add.at(incident, u, np.abs(wv))
    np.add.at(incident, v, np.abs(wv))
    return dict(resid=r, inv_den=inv_den, valid=valid, bone_valid=bone_valid, bone_resid=d, gcoef=gcoef, incident=incident,
                loss3=np.array([a0 * Bh[0] + a1 * Bh[1], Bh[0], Bh[1]]), acc=np.array([calls * Bh[0], calls * Bh[1], float(calls)]),
                dp=dp, bound=bound, bones=uv)


def bone_bound(ref):
    """(2, B, E, 2): bound_u + bound_v, the error allowed to the two residuals a bone subtracts."""
    u, v = ref["bones"][:, 0], ref["bones"][:, 1]
    return ref["bound"][:, :, u] + ref["bound"][:, :, v]


def sign_margin(ref):
    """The smallest |d| / (bound_u + bound_v) over both axes of every valid bone of both heads (inf when no bone is valid): at
    FACTOR = 50 or more no sign of d is decided by an fp32 residual's rounding."""
    ratio = (np.abs(ref["bone_resid"]) / bone_bound(ref))[:, ref["bone_valid"]]
    return float(ratio.min()) if ratio.size else np.inf
