"""CPU (-m "not gpu"): the integral coordinate loss at every layer short of a launch — ``TRAINING.coordLoss`` where the config is
read, the argument checks of hupr_coord_loss_fwd_f32 / hupr_coord_loss_bwd_f32 through ctypes, ``functional.CoordLossFn``'s argument
handling, the register / scratch metadata of csrc/coord_loss.hip — and the fp64 statement of the rule in include/hupr.h that
tests/test_coord_loss_gpu.py compares the kernels with (``ref_coord``).  The rule is new, so the reference is its own statement; it
is checked here against torch's fp64 autograd of the same forward and on hand-built planes.  The input generator of the GPU tests
(``make_case``) and the sign margin they assert (``sign_margin``) live here too, so that the seeds they fix can be checked without
a GPU (``test_the_fixed_seeds_leave_no_sign_to_rounding``)."""
import re

import numpy as np
import pytest
import torch

from listing import kernel_metadata

NAN, INF = float("nan"), float("inf")


# ---- the rule in fp64 ----------------------------------------------------------------------------------------------------------------
def ref_position(joints, stride, snap, H):
    """joints (B, K, 2) image pixels -> (a (B, K, 2) float64, valid (B, K) bool).  The position is the rule's own fp32 arithmetic
    (a division, and with snap an addition of 0.5 and a truncation), so it is taken in float32 and then held exactly in float64."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.asarray(joints, dtype=np.float32) / np.float32(stride)
        if snap:
            t = a + np.float32(0.5)
            ok = (t >= -2147483648.0) & (t < 2147483648.0)
            a = np.where(ok, np.trunc(np.where(ok, t, np.float32(0))), np.float32(NAN)).astype(np.float32)
        a = a.astype(np.float64)
        valid = (np.isfinite(a) & (a >= 0) & (a <= H - 1)).all(axis=-1)
    return a, valid


def ref_coord(p1, p2, joints, stride, snap, w=None, eps=1.0, a0=1.0, a1=1.0, g=1.0, calls=1):
    """The whole rule in fp64.  p1, p2: (B, K, H, H) arrays (taken as float64 exactly), joints (B, K, 2).  -> dict with loss3 =
    (a0 C_0 + a1 C_1, C_0, C_1), resid (2, B, K, 2), scale (2, B, K), valid (B, K), acc (3,) after ``calls`` calls, dp (2, B, K, H, H)
    by the stated backward rule for the gradient g of loss3[0], and A (2, B, K, 2) = sum p |x - a| / (S + eps), the magnitude the
    residual's error bound is relative to (0 for an invalid row)."""
    p = np.stack([np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)])
    _, B, K, H, _ = p.shape
    a, valid = ref_position(joints, stride, snap, H)
    wv = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    y, x = np.mgrid[0:H, 0:H].astype(np.float64)
    a_ = np.where(valid[..., None], a, 0.0)
    d = np.stack([x[None, None] - a_[..., 0, None, None], y[None, None] - a_[..., 1, None, None]])       # (2 axes, B, K, H, H)
    v5, v4, v3 = valid[None, :, :, None, None], valid[None, :, :, None], valid[None]
    with np.errstate(invalid="ignore"):
        pv = np.where(v5, p, 0.0)                                                                            # an invalid row's plane is not read
        den = pv.sum(axis=(-1, -2)) + eps                                                                    # (2, B, K)
        N = np.stack([(pv * d[0][None]).sum(axis=(-1, -2)), (pv * d[1][None]).sum(axis=(-1, -2))], axis=-1)  # (2, B, K, 2)
        A = np.stack([(pv * np.abs(d[0])[None]).sum(axis=(-1, -2)), (pv * np.abs(d[1])[None]).sum(axis=(-1, -2))], axis=-1)
        r = np.where(v4, N / den[..., None], 0.0)
        A = np.where(v4, A / den[..., None], 0.0)
        scale = np.where(v3, wv[None, None, :] / den, 0.0)
        l = np.where(v3, wv[None, None, :] * np.abs(r).sum(axis=-1), 0.0)
        C = l.sum(axis=(1, 2)) / (2 * B * K)
        G = g * np.array([a0, a1])
        f = G[:, None, None] * scale / (2 * B * K)
        dp = f[..., None, None] * (np.sign(r[..., 0])[..., None, None] * (d[0][None] - r[..., 0, None, None]) +
                                   np.sign(r[..., 1])[..., None, None] * (d[1][None] - r[..., 1, None, None]))
        dp = np.where((f == 0)[..., None, None], 0.0, dp)                                                  # a zero factor is written as zeros
    return dict(loss3=np.array([a0 * C[0] + a1 * C[1], C[0], C[1]]), resid=r, scale=scale, valid=valid, A=A,
                acc=np.array([calls * C[0], calls * C[1], float(calls)]), dp=dp)


def autograd_coord(p1, p2, joints, stride, snap, w=None, eps=1.0, a0=1.0, a1=1.0, g=1.0):
    """The same forward written in torch fp64 -> (loss3[0], its gradient times g with respect to both maps (2, B, K, H, H))."""
    p = torch.from_numpy(np.stack([np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)])).requires_grad_(True)
    _, B, K, H, _ = p.shape
    a, valid = ref_position(joints, stride, snap, H)
    a, valid = torch.from_numpy(np.where(valid[..., None], a, 0.0)), torch.from_numpy(valid)
    wv = torch.ones(K, dtype=torch.float64) if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="ij")
    pm = torch.where(valid[None, :, :, None, None], p, torch.zeros_like(p))
    den = pm.sum(dim=(-1, -2)) + eps
    rx = (pm * (xs - a[..., 0, None, None])).sum(dim=(-1, -2)) / den
    ry = (pm * (ys - a[..., 1, None, None])).sum(dim=(-1, -2)) / den
    l = torch.where(valid[None], wv * (rx.abs() + ry.abs()), torch.zeros_like(rx))
    C = l.sum(dim=(1, 2)) / (2 * B * K)
    loss = a0 * C[0] + a1 * C[1]
    (g * loss).backward()
    return loss.item(), p.grad.numpy()


def sign_margin(ref):
    """The smallest |r| over both axes of every valid row of both heads (inf when no row is valid)."""
    r = np.abs(ref["resid"])[:, ref["valid"]]
    return float(r.min()) if r.size else np.inf


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------
def make_case(B, K, H, seed, stride=4.0):
    """-> p1, p2 (B, K, H, H) float32, joints (B, K, 2) float32 in image pixels.  A map is noise clipped into [0, 0.2] plus one
    Gaussian bump of amplitude 0.8 on a random centre (sigma 2 at H = 64, at least 0.75), the two heads with their own noise around
    one bump.  A joint is the fp64 centroid of its two planes' sum plus, per axis, an offset of magnitude in [0.25, 6] heat-map px and
    random sign, clamped into the map, times ``stride``; an offset is drawn again while it leaves the centroid of either head within
    0.06 px of the joint or of the joint's nearest whole pixel on that axis."""
    rng = np.random.RandomState(seed)
    sigma = max(H / 32.0, 0.75)
    c = rng.uniform(0, H - 1, (B, K, 2))
    y, x = np.mgrid[0:H, 0:H].astype(np.float64)
    bump = 0.8 * np.exp(-((x[None, None] - c[..., 0, None, None]) ** 2 + (y[None, None] - c[..., 1, None, None]) ** 2) / (2 * sigma ** 2))
    ps = [(np.clip(rng.normal(0.1, 0.08, (B, K, H, H)), 0.0, 0.2) + bump).astype(np.float32) for _ in range(2)]
    both = ps[0].astype(np.float64) + ps[1].astype(np.float64)
    cen = np.stack([(both * x).sum(axis=(-1, -2)), (both * y).sum(axis=(-1, -2))], axis=-1) / both.sum(axis=(-1, -2))[..., None]
    # each head's own centroid and shrink S / (S + 1), to redraw an offset that leaves some |r| under 0.06 with snap 0 or 1 (the
    # tests assert MARGIN = 0.05 on the kernel's own rule; this only steers the draw, with eps = 1 as LossComputer passes it)
    S = [q.astype(np.float64).sum(axis=(-1, -2)) for q in ps]
    cens = [np.stack([(q * x).sum(axis=(-1, -2)), (q * y).sum(axis=(-1, -2))], axis=-1) / s[..., None] for q, s in zip(ps, S)]
    joints = np.zeros((B, K, 2), dtype=np.float32)
    todo = np.ones((B, K, 2), dtype=bool)
    for _ in range(200):
        off = rng.uniform(0.25, 6.0, (B, K, 2)) * rng.choice([-1.0, 1.0], (B, K, 2))
        cand = (np.clip(cen + off, 0.0, H - 1.0) * stride).astype(np.float32)
        joints = np.where(todo, cand, joints)
        a = joints.astype(np.float64) / stride
        small = np.zeros((B, K, 2), dtype=bool)
        for pos in (a, np.trunc(a + 0.5)):
            for c, s in zip(cens, S):
                small |= np.abs((c - pos) * (s / (s + 1.0))[..., None]) < 0.06
        todo = small
        if not todo.any():
            break
    return ps[0], ps[1], joints


def make_weights(K):
    """Per-joint weights with a zero and non-unit values (one weight of 2.0 when K = 1)."""
    if K == 1:
        return np.array([2.0], dtype=np.float32)
    w = np.random.RandomState(2000 + K).uniform(0.5, 2.0, K).astype(np.float32)
    w[K // 3] = 0.0
    return w


# (B, K, H) -> the seed of make_case, fixed so that with snap 0 and 1 every valid row of both heads has |r| >= MARGIN on both axes
# in fp64: (3, 14, 64) the model's shape, (1, 2, 128) the other configured map size with 64 terms per thread, (2, 17, 5) the 4-byte
# path, (33, 14, 8) many small rows, (1, 1, 5) the smallest problem
CASES = {(3, 14, 64): 0, (1, 2, 128): 0, (2, 17, 5): 0, (33, 14, 8): 0, (1, 1, 5): 0}
MARGIN = 0.05
STRIDE = 4.0
A0, A1, G = 0.3, 0.7, 1.7


def test_the_fixed_seeds_leave_no_sign_to_rounding():
    for (B, K, H), seed in CASES.items():
        p1, p2, joints = make_case(B, K, H, seed, STRIDE)
        assert p1.min() >= 0.0 and p1.max() <= 1.0 and p2.min() >= 0.0 and p2.max() <= 1.0
        for snap in (0, 1):
            ref = ref_coord(p1, p2, joints, STRIDE, snap)
            assert ref["valid"].all(), ((B, K, H), snap)                            # the joints are clamped into the map
            assert sign_margin(ref) >= MARGIN, ((B, K, H), seed, snap, sign_margin(ref))


# ---- the reference's own properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "B%d-K%d-H%d" % s)
def test_reference_backward_is_the_gradient_of_its_forward(shape):
    """The analytic dp of ref_coord against torch's fp64 autograd of the same forward: with and without snap, weights and a
    gradient and head weights that are not 1."""
    B, K, H = shape
    p1, p2, joints = make_case(B, K, H, CASES[shape], STRIDE)
    for snap in (0, 1):
        for w in (None, make_weights(K)):
            ref = ref_coord(p1, p2, joints, STRIDE, snap, w, 1.0, A0, A1, G)
            assert sign_margin(ref) >= MARGIN
            loss, grad = autograd_coord(p1, p2, joints, STRIDE, snap, w, 1.0, A0, A1, G)
            assert np.isclose(ref["loss3"][0], loss, rtol=1e-13, atol=0)
            assert np.allclose(ref["dp"], grad, rtol=1e-10, atol=0), np.abs(ref["dp"] - grad).max()
            if w is not None and K > 1:
                assert not ref["dp"][:, :, K // 3].any() and not ref["scale"][:, :, K // 3].any()


def test_reference_on_hand_built_planes():
    """One cell of mass m at (x, y) = (3, 1) on a 5 x 5 map, joint at heat-map (1.5, 2.25): r = m / (m + eps) times the offset; the
    invalid rows, the snap, the accumulator and the fixed denominator."""
    H, stride = 5, 4.0
    p = np.zeros((1, 3, H, H))
    p[0, 0, 1, 3] = 0.5
    p[0, 1, 1, 3] = 0.5
    p[0, 2] = NAN                                                                  # its joint is invalid: the plane is not read
    joints = np.array([[[6.0, 9.0], [6.0, 9.0], [6.0, -9.0]]])
    r = ref_coord(p, 2 * p, joints, stride, 0, np.array([1.0, 3.0, 1.0]), eps=1.0, a0=0.25, a1=2.0, g=1.0, calls=3)
    assert r["valid"].tolist() == [[True, True, False]]
    assert np.allclose(r["resid"][0, 0, 0], [0.5 / 1.5 * 1.5, 0.5 / 1.5 * -1.25], rtol=1e-15)
    assert np.allclose(r["resid"][1, 0, 0], [1.0 / 2.0 * 1.5, 1.0 / 2.0 * -1.25], rtol=1e-15)
    assert not r["resid"][:, 0, 2].any() and not r["scale"][:, 0, 2].any() and not r["dp"][:, 0, 2].any()
    assert np.allclose(r["scale"][0, 0], [1 / 1.5, 3 / 1.5, 0.0], rtol=1e-15)
    C0 = (1.0 + 3.0) * (0.5 / 1.5) * 2.75 / 6                                       # 2 B K = 6: the invalid row counts as a zero
    C1 = (1.0 + 3.0) * (1.0 / 2.0) * 2.75 / 6
    assert np.allclose(r["loss3"], [0.25 * C0 + 2.0 * C1, C0, C1], rtol=1e-14)
    assert np.allclose(r["acc"], [3 * C0, 3 * C1, 3.0], rtol=1e-14)
    assert np.isfinite(r["loss3"]).all() and np.isfinite(r["dp"]).all()
    # the bump's own cell: dp = G scale / 6 * (sgn(r_x) (x - a_x - r_x) + sgn(r_y) (y - a_y - r_y))
    want = 0.25 * (1 / 1.5) / 6 * ((3 - 1.5 - 0.5) - (1 - 2.25 + 1.25 / 3))
    assert np.isclose(r["dp"][0, 0, 0, 1, 3], want, rtol=1e-14)
    # snap: (int)(1.5 + 0.5) = 2, (int)(2.25 + 0.5) = 2; a joint just below zero snaps onto pixel 0 and is valid
    a, valid = ref_position(np.array([[[6.0, 9.0], [-1.0, 17.9], [18.1, 0.0], [NAN, 0.0], [INF, 0.0], [0.0, -INF], [3e10, 0.0]]]), stride, 1, H)
    assert valid.tolist() == [[True, True, False, False, False, False, False]]
    assert a[0, 0].tolist() == [2.0, 2.0] and a[0, 1].tolist() == [0.0, 4.0] and a[0, 2, 0] == 5.0
    _, valid = ref_position(np.array([[[16.0, 0.0], [16.1, 0.0], [-0.1, 0.0], [0.0, NAN]]]), stride, 0, H)
    assert valid.tolist() == [[True, False, False, False]]
    # an empty plane under a valid joint: r = 0 exactly, sgn(0) = 0, no gradient; a NaN cell in a valid plane is not masked
    z = ref_coord(np.zeros((1, 1, H, H)), np.zeros((1, 1, H, H)), np.array([[[6.0, 9.0]]]), stride, 0)
    assert not z["resid"].any() and not z["dp"].any() and z["scale"][0, 0, 0] == 1.0 and not z["loss3"].any()
    q = np.full((1, 2, H, H), 0.1)
    q[0, 1, 2, 2] = NAN
    n = ref_coord(q, np.full((1, 2, H, H), 0.1), np.array([[[6.0, 9.0], [6.0, 9.0]]]), stride, 0)
    assert np.isnan(n["loss3"][:2]).all() and np.isfinite(n["loss3"][2]) and np.isnan(n["resid"][0, 0, 1]).all()
    assert np.isfinite(n["resid"][0, 0, 0]).all() and np.isnan(n["dp"][0, 0, 1]).all() and np.isfinite(n["dp"][0, 0, 0]).all()


# ---- the setting ---------------------------------------------------------------------------------------------------------------------
def _cfg(**training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    return cfg


def test_coord_loss_is_validated_where_the_config_is_read():
    from hupr_amd.misc.losses import LossComputer, coord_loss_setting
    cfg = _cfg()
    assert not hasattr(cfg.TRAINING, "coordLoss")                                   # the shipped YAML is the reference's
    assert coord_loss_setting(cfg) is None and coord_loss_setting(_cfg(coordLoss=-1)) is None
    assert coord_loss_setting(_cfg(coordLoss=-1.0)) is None
    for off in (cfg, _cfg(coordLoss=-1)):
        lc = LossComputer(off, "cpu")
        assert lc.coordLoss is None and lc.coord_acc is None and lc.coord_residual is None
    for lam in (0.5, 1, 2, 1e-3, 100.0):
        got = coord_loss_setting(_cfg(coordLoss=lam))
        assert got == lam and isinstance(got, float)
        lc = LossComputer(_cfg(coordLoss=lam), "cpu")
        assert lc.coordLoss == lam and lc.coord_residual is None and not lc.mined
        assert lc.coord_acc.dtype == torch.float64 and tuple(lc.coord_acc.shape) == (3,) and not lc.coord_acc.any()
    for bogus in (0, 0.0, -2, -0.5, NAN, INF, -INF, True, False, "0.5", "", None, [0.5], {"weight": 0.5}):
        with pytest.raises(ValueError) as e:
            coord_loss_setting(_cfg(coordLoss=bogus))
        assert "TRAINING.coordLoss" in str(e.value)
        with pytest.raises(ValueError):
            LossComputer(_cfg(coordLoss=bogus), "cpu")


# ---- the C ABI and the Function, short of a launch -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


P = 4096                                                   # any non-null address: every call below returns before it launches


def _fwd(L, p1=P, p2=P, joints=P, B=3, K=14, H=64, stride=4.0, snap=0, w=None, eps=1.0, loss3=P, resid=P, scale=P, acc=None):
    return L.hupr_coord_loss_fwd_f32(p1, p2, joints, B, K, H, stride, snap, w, eps, 1.0, 1.0, loss3, resid, scale, acc, None)


def _bwd(L, resid=P, scale=P, joints=P, g=P, B=3, K=14, H=64, stride=4.0, snap=0, dp1=P, dp2=P):
    return L.hupr_coord_loss_bwd_f32(resid, scale, joints, g, B, K, H, stride, snap, 1.0, 1.0, dp1, dp2, None)


def test_entry_points_check_their_arguments_on_the_host(L):
    n0 = L.hupr_launch_count()
    shapes = [dict(B=0), dict(B=-3), dict(K=0), dict(K=65), dict(K=-14), dict(H=0), dict(H=-64), dict(H=4097), dict(B=1 << 60),
              dict(B=1 << 50, H=4096), dict(stride=0.0), dict(stride=-4.0), dict(stride=NAN), dict(stride=INF)]
    fwd_refused = [dict(p1=None), dict(p2=None), dict(joints=None), dict(loss3=None), dict(resid=None), dict(scale=None),
                   dict(eps=0.0), dict(eps=-1.0), dict(eps=NAN), dict(eps=INF)] + shapes
    for kw in fwd_refused:
        assert _fwd(L, **kw) == -1, kw
        msg = L.hupr_last_error()
        assert msg.startswith(b"hupr_coord_loss_fwd_f32: ") and len(msg) > 36, (kw, msg)
    bwd_refused = [dict(resid=None), dict(scale=None), dict(joints=None), dict(g=None), dict(dp1=None), dict(dp2=None)] + shapes
    for kw in bwd_refused:
        assert _bwd(L, **kw) == -1, kw
        msg = L.hupr_last_error()
        assert msg.startswith(b"hupr_coord_loss_bwd_f32: ") and len(msg) > 36, (kw, msg)
    assert _fwd(L, p1=None) == -1 and b"null" in L.hupr_last_error()
    assert _fwd(L, K=65) == -1 and b"K 65" in L.hupr_last_error()
    assert _fwd(L, H=4097) == -1 and b"H 4097" in L.hupr_last_error()
    assert _fwd(L, eps=0.0) == -1 and b"eps" in L.hupr_last_error()
    assert _bwd(L, stride=0.0) == -1 and b"stride" in L.hupr_last_error()
    assert _bwd(L, scale=None) == -1 and b"null" in L.hupr_last_error()
    assert L.hupr_launch_count() == n0                        # refused before any launch


def test_function_refuses_what_it_cannot_run():
    from hupr_amd import functional as F_
    import __graft_entry__ as g
    g.build()
    x, j = torch.full((2, 14, 8, 8), 0.5), torch.zeros((2, 14, 2))
    for args in ((x, x, j, 4.0, False, None, 1.0, 1.0, None),                          # CPU tensors: no fallback
                 (x.double(), x.double(), j, 4.0, False, None, 1.0, 1.0, None),
                 (x.numpy(), x, j, 4.0, False, None, 1.0, 1.0, None)):
        with pytest.raises(ValueError):
            F_.CoordLossFn.apply(*args)


def test_coord_loss_kernels_use_no_scratch():
    """The listing the build keeps for csrc/coord_loss.hip: the plane and backward kernels in their 16-byte and 4-byte forms and the
    sum kernel, nothing else; 0 spilled registers, 0 bytes of scratch, 256 threads, at most 64 VGPRs (eight waves per SIMD fit)."""
    meta = kernel_metadata("coord_loss")
    kinds = sorted(re.search(r"hupr_k_coord_loss_[a-z]+(ILb[01]E)?", name).group(0) for name in meta)
    assert kinds == ["hupr_k_coord_loss_bwdILb0E", "hupr_k_coord_loss_bwdILb1E", "hupr_k_coord_loss_planeILb0E",
                     "hupr_k_coord_loss_planeILb1E", "hupr_k_coord_loss_sum"], sorted(meta)
    for name, m in meta.items():
        assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0, (name, m)
        assert m["threads"] == 256 and m["vgpr"] <= 64 and m["lds"] <= 1024, (name, m)
