"""CPU (-m "not gpu"): online hard keypoint mining and per-joint weights at every layer short of a launch — ``TRAINING.ohkm`` and
``TRAINING.jointWeights`` where the config is read, the argument checks of hupr_bce_mined_fwd_f32 / hupr_bce_mined_bwd_f32 through
ctypes, ``functional.MinedBCEFn``'s argument handling, the register / scratch metadata of csrc/bce_mined.hip — and the fp64
statement of the rule in include/hupr.h that tests/test_ohkm_gpu.py compares the kernels with (``ref_mined``), checked here against
``torch.nn.functional.binary_cross_entropy`` and on hand-built ties and NaNs.  The input generator of the GPU tests (``make_case``)
and the selection margin they assert (``selection_margin``) live here too, so that the seeds they fix can be checked without a GPU
(``test_the_fixed_seeds_leave_no_selection_to_rounding``)."""
import copy
import re

import numpy as np
import pytest
import torch

from listing import kernel_metadata


# ---- the rule in fp64 ----------------------------------------------------------------------------------------------------------------
def ref_plane_loss(p, t):
    """p, t (..., HW) float64 tensors -> the plane means of -(t log p + (1 - t) log(1 - p)), both logs clamped at -100."""
    return -(t * torch.log(p).clamp(min=-100.0) + (1.0 - t) * torch.log(1.0 - p).clamp(min=-100.0)).mean(dim=-1)


def ref_select(v, k):
    """v (..., K) float64 ndarray -> bool mask of the first k planes ordered by v descending, a NaN above every number, equal values
    and two NaNs by lower joint index: a stable sort on (-v, index) with NaN keyed as -inf."""
    key = np.where(np.isnan(v), -np.inf, -v)
    order = np.argsort(key, axis=-1, kind="stable")
    sel = np.zeros(v.shape, dtype=bool)
    np.put_along_axis(sel, order[..., :k], True, axis=-1)
    return sel


def ref_mined(p1, p2, t, k, w=None, alpha=1.0, beta=1.0, g=1.0, g2=None):
    """The whole rule in fp64.  p1, p2, t: (B, K, HW) arrays (taken as float64 exactly).  -> dict with plane_loss (2, B, K), v, sel
    (bool), loss3 = (alpha L_0 + beta L_1, L_0, L_1), coef (2, B, K), counts (2, K), and the gradients dp1, dp2 of
    g * loss3[0] + g2 * loss3[2] twice: by autograd through the losses (``dp_autograd``) and by the stated backward rule with its
    1e-12 floor (``dp_rule``); the two differ only where a clamp or the floor acts (p exactly 0 or 1)."""
    p = torch.from_numpy(np.stack([np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)])).requires_grad_(True)
    T = torch.from_numpy(np.asarray(t, dtype=np.float64))
    _, B, K, HW = p.shape
    wv = torch.ones(K, dtype=torch.float64) if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64))
    l = ref_plane_loss(p, T[None])
    v = wv * l
    sel = ref_select(v.detach().numpy(), k)
    st = torch.from_numpy(sel)
    L = torch.where(st, v, torch.zeros_like(v)).sum(dim=(1, 2)) / (B * k)                 # no gradient through the selection
    loss = alpha * L[0] + beta * L[1]
    total = g * loss + (g2 * L[1] if g2 is not None else 0.0)
    finite = bool(torch.isfinite(total))
    if finite:
        total.backward()
    coef = np.where(sel, wv.numpy() / (B * k * HW), 0.0)
    G = np.array([g * alpha, g * beta + (g2 if g2 is not None else 0.0)])
    pd, td = p.detach().numpy(), T.numpy()[None]
    rule = G[:, None, None, None] * coef[..., None] * (pd - td) / np.maximum(pd * (1.0 - pd), 1e-12)
    return dict(plane_loss=l.detach().numpy(), v=v.detach().numpy(), sel=sel, loss3=np.array([loss.item(), L[0].item(), L[1].item()]),
                coef=coef, counts=sel.sum(axis=1).astype(np.int64), dp_autograd=p.grad.numpy() if finite else None, dp_rule=rule)


def selection_margin(v, k):
    """The smallest relative gap between the k-th and the (k + 1)-th largest v over all (head, sample); inf for k = K."""
    s = -np.sort(-v, axis=-1)
    if k >= v.shape[-1]:
        return np.inf
    return float(((s[..., k - 1] - s[..., k]) / s[..., k - 1]).min())


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------
def make_case(B, K, H, seed):
    """-> p1, p2, t (B, K, H * H) float32.  t: a Gaussian of amplitude 1 on a random centre (sigma 2 at H = 64, at least 0.75);
    p_h = clip(t + s_h a[b, j] u_h, 1e-4, 1 - 1e-4) with u uniform in (-1, 1), a[b] a permutation of linspace(0.05, 0.6, K) drawn
    per sample, s = (1, 0.8): every plane has its own difficulty, so the planes' losses are far apart."""
    rng = np.random.RandomState(seed)
    sigma = max(H / 32.0, 0.75)
    c = rng.uniform(0, H - 1, (B, K, 2))
    y, x = np.mgrid[0:H, 0:H]
    t = np.exp(-((x[None, None] - c[..., 0, None, None]) ** 2 + (y[None, None] - c[..., 1, None, None]) ** 2) / (2 * sigma ** 2))
    t = t.reshape(B, K, H * H).astype(np.float32)
    a = np.stack([rng.permutation(np.linspace(0.05, 0.6, K)) for _ in range(B)])
    ps = []
    for s in (1.0, 0.8):
        u = rng.uniform(-1.0, 1.0, (B, K, H * H))
        ps.append(np.clip(t + s * a[..., None] * u, 1e-4, 1.0 - 1e-4).astype(np.float32))
    return ps[0], ps[1], t


def make_weights(K):
    """Per-joint weights with a zero and non-unit values (one weight of 2.0 when K = 1)."""
    if K == 1:
        return np.array([2.0], dtype=np.float32)
    w = np.random.RandomState(1000 + K).uniform(0.5, 2.0, K).astype(np.float32)
    w[K // 3] = 0.0
    return w


# (B, K, H) -> the seed of make_case, fixed so that for every k in ks(K), with and without make_weights(K), the k-th and (k + 1)-th
# largest v of every (head, sample) differ by at least MARGIN relative in fp64
CASES = {(3, 14, 64): 0, (2, 17, 5): 0, (2, 64, 5): 0, (33, 14, 8): 15, (1, 1, 5): 0}
MARGIN = 1e-3


def ks(K):
    return sorted({1, max(K // 2, 1), max(K - 1, 1), K})


def test_the_fixed_seeds_leave_no_selection_to_rounding():
    for (B, K, H), seed in CASES.items():
        p1, p2, t = make_case(B, K, H, seed)
        for w in (None, make_weights(K)):
            v = ref_mined(p1, p2, t, K, w)["v"]
            for k in ks(K):
                assert selection_margin(v, k) >= MARGIN, ((B, K, H), seed, k, w is not None, selection_margin(v, k))


# ---- the reference's own properties ------------------------------------------------------------------------------------------------------
def test_reference_with_every_joint_kept_is_binary_cross_entropy():
    import torch.nn.functional as F
    B, K, H = 3, 14, 8
    p1, p2, t = make_case(B, K, H, 5)
    r = ref_mined(p1, p2, t, K, None, alpha=0.3, beta=0.7, g=1.7, g2=0.5)
    a1 = torch.from_numpy(p1).double().requires_grad_(True)
    a2 = torch.from_numpy(p2).double().requires_grad_(True)
    T = torch.from_numpy(t).double()
    l1, l2 = F.binary_cross_entropy(a1, T), F.binary_cross_entropy(a2, T)
    (1.7 * (0.3 * l1 + 0.7 * l2) + 0.5 * l2).backward()
    assert np.allclose(r["loss3"], [0.3 * l1.item() + 0.7 * l2.item(), l1.item(), l2.item()], rtol=1e-13, atol=0)
    assert r["sel"].all() and np.array_equal(r["counts"], np.full((2, K), B))
    assert np.allclose(r["coef"], 1.0 / (B * K * H * H), rtol=1e-15, atol=0)
    for got in (r["dp_autograd"], r["dp_rule"]):
        assert np.allclose(got[0], a1.grad.numpy(), rtol=1e-11, atol=0) and np.allclose(got[1], a2.grad.numpy(), rtol=1e-11, atol=0)
    per_plane = F.binary_cross_entropy(a1, T, reduction="none").mean(dim=-1)
    assert np.allclose(r["plane_loss"][0], per_plane.detach().numpy(), rtol=1e-13, atol=0)


def test_reference_keeps_the_k_largest_weighted_planes():
    B, K, H = 2, 6, 5
    p1, p2, t = make_case(B, K, H, 7)
    w = np.array([1.0, 0.0, 3.0, 0.5, 1.0, 2.0])
    r = ref_mined(p1, p2, t, 2, w, alpha=0.25, beta=2.0, g=1.0, g2=None)
    v = r["v"]
    assert np.allclose(v, w * r["plane_loss"], rtol=1e-15, atol=0)
    for h in range(2):
        for b in range(B):
            top = set(torch.topk(torch.from_numpy(v[h, b]), 2).indices.tolist())
            assert set(np.flatnonzero(r["sel"][h, b])) == top and 1 not in top
    L = [np.where(r["sel"][h], v[h], 0.0).sum() / (B * 2) for h in range(2)]
    assert np.allclose(r["loss3"], [0.25 * L[0] + 2.0 * L[1], L[0], L[1]], rtol=1e-14, atol=0)
    assert (r["coef"][~r["sel"]] == 0).all() and np.allclose(r["coef"][r["sel"]], np.broadcast_to(w, v.shape)[r["sel"]] / (B * 2 * H * H))
    assert r["counts"].sum() == 2 * B * 2 and (r["counts"][:, 1] == 0).all()
    # no gradient outside the kept planes, and none through the selection: the kept planes' gradient is that of their own mean
    assert (r["dp_autograd"][~r["sel"]] == 0).all() and (r["dp_rule"][~r["sel"]] == 0).all()
    assert np.allclose(r["dp_autograd"], r["dp_rule"], rtol=1e-11, atol=0)


def test_reference_tie_rule_and_nan_rank():
    v = np.array([[1.0, 3.0, 3.0, 0.5, 3.0]])
    assert np.array_equal(ref_select(v, 1), [[False, True, False, False, False]])
    assert np.array_equal(ref_select(v, 2), [[False, True, True, False, False]])
    assert np.array_equal(ref_select(v, 4), [[True, True, True, False, True]])
    nan = float("nan")
    v = np.array([[5.0, nan, 100.0, nan, 0.0]])
    assert np.array_equal(ref_select(v, 1), [[False, True, False, False, False]])           # a NaN above every number, lower index first
    assert np.array_equal(ref_select(v, 2), [[False, True, False, True, False]])
    assert np.array_equal(ref_select(v, 3), [[False, True, True, True, False]])
    assert np.array_equal(ref_select(np.zeros((1, 4)), 2), [[True, True, False, False]])     # all equal (e.g. weights of zero)
    # through the whole rule: two identical planes tie, one NaN cell makes its plane first and the loss NaN
    p1, p2, t = make_case(1, 4, 5, 3)
    p1[0, 3], t[0, 3] = p1[0, 1], t[0, 1]
    l = ref_mined(p1, p2, t, 1)["plane_loss"][0, 0]
    assert l[1] == l[3]
    k = int((l > l[1]).sum()) + 1                                                        # cuts between the two tied planes
    sel = ref_mined(p1, p2, t, k)["sel"][0, 0]
    assert sel[1] and not sel[3] and sel.sum() == k
    p1[0, 2, 7] = nan
    r = ref_mined(p1, p2, t, 1)
    assert np.flatnonzero(r["sel"][0, 0]).tolist() == [2] and np.isnan(r["loss3"][0]) and np.isnan(r["loss3"][1])
    assert np.isfinite(r["loss3"][2]) and np.isfinite(np.delete(r["plane_loss"][0, 0], 2)).all()


def test_reference_clamps_and_floor():
    """p exactly 0 and 1 against t in {0, 1}: the -100 clamp of the forward and the 1e-12 floor of the backward."""
    p = np.array([[[0.0, 0.0, 1.0, 1.0, 0.5]]])
    t = np.array([[[0.0, 1.0, 0.0, 1.0, 1.0]]])
    r = ref_mined(p, p, t, 1, None, g=1.0)
    assert np.isclose(r["plane_loss"][0, 0, 0], (0.0 + 100.0 + 100.0 + 0.0 + np.log(2.0)) / 5, rtol=1e-15)
    want = np.array([0.0, -1e12, 1e12, 0.0, -2.0]) / 5
    assert np.allclose(r["dp_rule"][0, 0, 0], want, rtol=1e-15, atol=0)


# ---- the two settings ------------------------------------------------------------------------------------------------------------------
def _cfg(**training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    return cfg


def test_ohkm_is_validated_where_the_config_is_read():
    from hupr_amd.misc.losses import LossComputer, ohkm_setting
    cfg = _cfg()
    assert not hasattr(cfg.TRAINING, "ohkm") and not hasattr(cfg.TRAINING, "jointWeights")       # the shipped YAML is the reference's
    assert ohkm_setting(cfg) is None
    lc = LossComputer(cfg, "cpu")
    assert lc.ohkm is None and lc.jointWeights is None and not lc.mined and lc.mining_counts is None
    assert ohkm_setting(_cfg(ohkm=-1)) is None and not LossComputer(_cfg(ohkm=-1), "cpu").mined
    K = cfg.DATASET.numKeypoints
    for k in (1, 8, K):
        assert ohkm_setting(_cfg(ohkm=k)) == k
        lc = LossComputer(_cfg(ohkm=k), "cpu")
        assert lc.mined and lc.mined_k == k and lc.jointWeights is None
        assert lc.mining_counts.dtype == torch.int64 and tuple(lc.mining_counts.shape) == (2, K) and not lc.mining_counts.any()
    for bogus in (0, -2, K + 1, 100, True, False, 8.0, -1.0, float("nan"), "8", "", None, [8]):
        with pytest.raises(ValueError) as e:
            ohkm_setting(_cfg(ohkm=bogus))
        assert "TRAINING.ohkm" in str(e.value)
        with pytest.raises(ValueError):
            LossComputer(_cfg(ohkm=bogus), "cpu")
    small = _cfg(ohkm=8)
    small.DATASET = copy.copy(small.DATASET)
    small.DATASET.numKeypoints = 7                                                                # the range follows the data set
    with pytest.raises(ValueError):
        ohkm_setting(small)


def test_joint_weights_are_validated_where_the_config_is_read():
    from hupr_amd.misc.losses import LossComputer, joint_weights_setting
    K = _cfg().DATASET.numKeypoints
    assert joint_weights_setting(_cfg()) is None and joint_weights_setting(_cfg(jointWeights=-1)) is None
    good = [1.0] * (K - 4) + [1.5, 1.5, 2, 0]
    got = joint_weights_setting(_cfg(jointWeights=good))
    assert got == [float(x) for x in good] and all(isinstance(x, float) for x in got)
    lc = LossComputer(_cfg(jointWeights=good), "cpu")
    assert lc.mined and lc.ohkm is None and lc.mined_k == K and lc.jointWeights == got        # weights alone: every joint kept
    lc = LossComputer(_cfg(jointWeights=good, ohkm=8), "cpu")
    assert lc.mined and lc.mined_k == 8 and lc.jointWeights == got
    inf, nan = float("inf"), float("nan")
    for bogus in ([1.0] * (K - 1), [1.0] * (K + 1), [], [0.0] * K, [1.0] * (K - 1) + [-0.5], [1.0] * (K - 1) + [nan],
                  [1.0] * (K - 1) + [inf], [1.0] * (K - 1) + ["1"], [1.0] * (K - 1) + [True], [1.0] * (K - 1) + [None],
                  0, 1, 1.0, -2, True, "1", None, {"Neck": 1.0}):
        with pytest.raises(ValueError) as e:
            joint_weights_setting(_cfg(jointWeights=bogus))
        assert "TRAINING.jointWeights" in str(e.value)
        with pytest.raises(ValueError):
            LossComputer(_cfg(jointWeights=bogus), "cpu")


# ---- the C ABI and the Function, short of a launch -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


P = 4096                                                   # any non-null address: every call below returns before it launches


def _fwd(L, p1=P, p2=P, t=P, B=3, K=14, HW=4096, k=8, w=None, loss3=P, plane_loss=P, coef=P, counts=None):
    return L.hupr_bce_mined_fwd_f32(p1, p2, t, B, K, HW, k, w, 1.0, 1.0, loss3, plane_loss, coef, counts, None)


def _bwd(L, p1=P, p2=P, t=P, coef=P, g=P, g2=None, dp1=P, dp2=P, B=3, K=14, HW=4096):
    return L.hupr_bce_mined_bwd_f32(p1, p2, t, coef, g, g2, 1.0, 1.0, dp1, dp2, B, K, HW, None)


def test_entry_points_check_their_arguments_on_the_host(L):
    n0 = L.hupr_launch_count()
    fwd_refused = [dict(p1=None), dict(p2=None), dict(t=None), dict(loss3=None), dict(plane_loss=None), dict(coef=None),
                   dict(k=0), dict(k=-1), dict(k=15), dict(K=65, k=8), dict(K=65, k=65), dict(K=0, k=0), dict(K=-14),
                   dict(B=0), dict(B=-3), dict(HW=0), dict(HW=-4096), dict(B=1 << 60), dict(HW=1 << 60), dict(B=1 << 40, HW=1 << 40)]
    for kw in fwd_refused:
        assert _fwd(L, **kw) == -1, kw
        msg = L.hupr_last_error()
        assert msg.startswith(b"hupr_bce_mined_fwd_f32: ") and len(msg) > 35, (kw, msg)
    bwd_refused = [dict(p1=None), dict(p2=None), dict(t=None), dict(coef=None), dict(g=None), dict(dp1=None), dict(dp2=None),
                   dict(K=65), dict(K=0), dict(B=0), dict(HW=0), dict(B=1 << 60), dict(HW=1 << 60)]
    for kw in bwd_refused:
        assert _bwd(L, **kw) == -1, kw
        msg = L.hupr_last_error()
        assert msg.startswith(b"hupr_bce_mined_bwd_f32: ") and len(msg) > 35, (kw, msg)
    assert _fwd(L, p1=None) == -1 and b"null" in L.hupr_last_error()
    assert _fwd(L, k=0) == -1 and b"k 0" in L.hupr_last_error()
    assert _fwd(L, k=15) == -1 and b"k 15" in L.hupr_last_error() and b"14" in L.hupr_last_error()
    assert _fwd(L, K=65, k=8) == -1 and b"K 65" in L.hupr_last_error()
    assert _bwd(L, coef=None) == -1 and b"null" in L.hupr_last_error()
    assert _bwd(L, K=65) == -1 and b"K 65" in L.hupr_last_error()
    assert L.hupr_launch_count() == n0                        # refused before any launch


def test_function_refuses_what_it_cannot_run():
    from hupr_amd import functional as F_
    import __graft_entry__ as g
    g.build()
    x = torch.full((2, 14, 8, 8), 0.5)
    for args in ((x, x, x, 8, None, 1.0, 1.0, None),                                     # CPU tensors: no fallback
                 (x.double(), x.double(), x.double(), 8, None, 1.0, 1.0, None),
                 (x.numpy(), x, x, 8, None, 1.0, 1.0, None)):
        with pytest.raises(ValueError):
            F_.MinedBCEFn.apply(*args)


def test_mined_kernels_use_no_scratch():
    """The listing the build keeps for csrc/bce_mined.hip: the plane and backward kernels in their 16-byte and 4-byte forms and the
    selection kernel, nothing else; 0 spilled registers, 0 bytes of scratch, 256 threads, at most 64 VGPRs (eight waves per SIMD fit)."""
    meta = kernel_metadata("bce_mined")
    kinds = sorted(re.search(r"hupr_k_bce_mined_[a-z]+(ILb[01]E)?", name).group(0) for name in meta)
    assert kinds == ["hupr_k_bce_mined_bwdILb0E", "hupr_k_bce_mined_bwdILb1E", "hupr_k_bce_mined_planeILb0E",
                     "hupr_k_bce_mined_planeILb1E", "hupr_k_bce_mined_select"], sorted(meta)
    for name, m in meta.items():
        assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0, (name, m)
        assert m["threads"] == 256 and m["vgpr"] <= 64 and m["lds"] <= 8 * 1024, (name, m)
