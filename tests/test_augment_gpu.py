"""GPU (-m gpu): the radar augmentation kernels (csrc/augment.hip) against torch / the host restatement in tools/augment.py, the
training path of TrainEngine with the TRAINING.aug* keys (eager, captured and replayed), the flip test, and the Runner."""
import ctypes
import os

import numpy as np
import pytest
import torch

from hupr_amd import synth
from hupr_amd.tools import augment as aug

pytestmark = pytest.mark.gpu

G = 8
PAIRS = [3, 4, 5, 0, 1, 2, 6, 7, 11, 12, 13, 8, 9, 10]


def _dev():
    return torch.device("cuda", 0)


def _rt():
    from hupr_amd import runtime as rt
    return rt


def _cfg(test=None, **training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    for k, v in (test or {}).items():
        setattr(cfg.TEST, k, v)
    return cfg


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the ADC mirror ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cubes():
    """3 G frames, their host permutation, and both on the device (computed once, never modified)."""
    host = synth.adc_cube_int16(31, nframes=3 * G)
    host_m = aug.mirror_adc_host(host)
    return host, host_m, torch.from_numpy(host).to(_dev()), torch.from_numpy(host_m).to(_dev())


def _torch_mirror(adc):
    c = torch.arange(192, device=adc.device)
    return adc.flip(1)[:, :, c + 2 - 2 * (c % 3)]


def test_adc_mirror_equals_torch_indexing(cubes):
    host, host_m, adc, adc_m = cubes
    keep = adc.clone()
    flags = torch.tensor([1, 0, 1], dtype=torch.uint8, device=_dev())
    out = aug.adc_mirror(adc, flags, G)
    want = adc.clone()
    want[:G], want[2 * G:] = _torch_mirror(adc[:G]), _torch_mirror(adc[2 * G:])
    assert out.dtype == torch.int16 and out.shape == adc.shape and out.data_ptr() != adc.data_ptr()
    assert torch.equal(out, want)
    assert torch.equal(out[G:2 * G], adc[G:2 * G]) and not torch.equal(out[:G], adc[:G])
    assert torch.equal(adc, keep)                                                   # the source is unchanged
    every = aug.adc_mirror(adc)                                                     # null flags: every frame
    assert torch.equal(every, _torch_mirror(adc)) and torch.equal(every, adc_m)
    assert torch.equal(aug.adc_mirror(out, flags, G), adc) and torch.equal(aug.adc_mirror(every), adc)      # twice = the identity
    assert torch.equal(aug.adc_mirror(adc, torch.zeros(3 * G, dtype=torch.uint8, device=_dev()), 1), adc)
    per_frame = torch.zeros(3 * G, dtype=torch.uint8, device=_dev())
    per_frame[5] = 1
    one = aug.adc_mirror(adc, per_frame, 1)
    assert torch.equal(one[5], adc_m[5]) and torch.equal(one[:5], adc[:5]) and torch.equal(one[6:], adc[6:])


def test_fft_chain_of_the_mirrored_buffer_equals_that_of_the_host_permuted_cube(cubes):
    from hupr_amd.preprocessing.process_iwr1843 import fft_chain_loader_means
    _, _, adc, adc_m = cubes
    flags = torch.tensor([1, 0, 1], dtype=torch.uint8, device=_dev())
    got = fft_chain_loader_means(aug.adc_mirror(adc, flags, G))
    want = fft_chain_loader_means(torch.cat([adc_m[:G], adc[G:2 * G], adc_m[2 * G:]]))
    assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(got[:G], fft_chain_loader_means(adc)[:G])


def test_adc_mirror_argument_errors_launch_nothing(cubes):
    rt = _rt()
    L, s = rt.lib(), None
    adc = cubes[2]
    out = torch.full_like(adc[:2], 7)
    p, o = adc.data_ptr(), out.data_ptr()
    n0 = L.hupr_launch_count()
    assert L.hupr_adc_mirror_i16(None, None, 0, 1, None, s) == 0                    # an empty batch is a no-op
    for args in ((None, o, 2, 1), (p, None, 2, 1), (p, o, -1, 1), (p, o, 2, 0), (p, o, 3, 2), (p, p, 2, 1), (p, p + 786432, 2, 1),
                 (p + 2, o, 2, 1), (p, o + 8, 1, 1)):
        assert L.hupr_adc_mirror_i16(args[0], args[1], args[2], args[3], None, s) == -1, args
        assert b"hupr_adc_mirror_i16" in L.hupr_last_error()
    assert L.hupr_launch_count() == n0
    with pytest.raises(ValueError):
        aug.adc_mirror(adc.float())
    with pytest.raises(ValueError):
        aug.adc_mirror(adc, torch.zeros(5, dtype=torch.uint8, device=_dev()), G)
    with pytest.raises(rt.HuprError):
        aug.adc_mirror(adc.cpu())
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
SETTINGS = dict(augMirror=0.5, augNoise=0.75, augMaskRange=12, augMaskAngle=20)


def _augmenter(seed, rank=0, **training):
    cfg = _cfg(**(training or SETTINGS))
    return aug.Augmenter(cfg, aug.augment_settings(cfg), _dev(), seed=seed, rank=rank)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("seed", [0, 20261019])
def test_plan_equals_the_host_plan(B, seed):
    a = _augmenter(seed, rank=3)
    st = a.stats()
    assert st == {"steps": 0, "samples": 0, "mirrored": 0, "mean_sigma": 0.0, "last_plan": None}
    mirrored, sigma_sum = 0, 0.0
    for step in range(3):
        a.plan(B)
        table, flags = a.table.cpu().numpy(), a.flags.cpu().numpy()
        want, want_flags = aug.plan_reference(B, step, seed, 3, 0.5, 0.75, 12, 20, 64, 64)
        ints = [c for c in range(8) if c != aug.SIGMA]
        assert np.array_equal(table[:, ints], want[:, ints]) and np.array_equal(flags, want_flags)
        s_got, s_want = aug.plan_sigma(table), aug.plan_sigma(want)
        assert (np.abs(s_got - s_want) <= np.spacing(s_want)).all() and (s_got >= 0).all() and (s_got < 0.75).all()
        mirrored += int(flags.sum())
        for s in s_got:
            sigma_sum += float(s)
        st = a.stats()
        assert st["steps"] == step + 1 and st["samples"] == B * (step + 1) and st["mirrored"] == mirrored
        assert st["mean_sigma"] == sigma_sum / (B * (step + 1))                     # fp64 adds in sample order
        assert np.array_equal(st["last_plan"], table)
    a.set_step((1 << 32) + 1)                                                       # resume; the high word of the counter counts
    a.plan(B)
    assert np.array_equal(a.table.cpu().numpy()[:, 2:], aug.plan_reference(B, (1 << 32) + 1, seed, 3, 0.5, 0.75, 12, 20, 64, 64)[0][:, 2:])
    assert a.stats()["steps"] == (1 << 32) + 2 and a.stats()["samples"] == B


def test_one_seed_gives_one_plan_and_ranks_differ():
    a, b, c, d = _augmenter(7), _augmenter(7), _augmenter(7, rank=1), _augmenter(8)
    for x in (a, b, c, d):
        x.plan(64)
    assert torch.equal(a.table, b.table) and torch.equal(a.flags, b.flags)
    assert not torch.equal(a.table, c.table) and not torch.equal(a.table, d.table)
    first = a.table.clone()
    a.plan(64)
    assert not torch.equal(a.table, first)                                          # the counter moved: a fresh plan
    fl = first[:, aug.MIRROR].sum().item()
    assert 0 < fl < 64
    lens = first[:, [aug.RANGE_LEN, aug.HORI_LEN, aug.VERT_LEN]]
    assert lens.min().item() >= 0 and first[:, aug.RANGE_LEN].max().item() <= 12 and lens.max().item() <= 20
    assert not torch.equal(first[:, aug.HORI_LEN], first[:, aug.VERT_LEN])


def test_plan_argument_errors_launch_nothing():
    rt = _rt()
    L = rt.lib()
    st = torch.zeros(4, dtype=torch.int64, device=_dev())
    tb = torch.zeros((4, 8), dtype=torch.int32, device=_dev())
    fl = torch.zeros(4, dtype=torch.uint8, device=_dev())
    ok = dict(B=4, st=st.data_ptr(), p=0.5, s=1.0, mr=8, ma=8, R=64, A=64, seed=1, rank=0, tb=tb.data_ptr(), fl=fl.data_ptr())
    n0 = L.hupr_launch_count()
    for bad in (dict(B=0), dict(B=65536), dict(st=None), dict(tb=None), dict(fl=None), dict(st=st.data_ptr() + 4), dict(p=-0.1), dict(p=1.5),
                dict(p=float("nan")), dict(s=-1.0), dict(s=float("inf")), dict(s=float("nan")), dict(mr=-1), dict(mr=33), dict(ma=33),
                dict(R=0), dict(A=0), dict(rank=-1), dict(rank=1 << 30)):
        a = dict(ok, **bad)
        assert L.hupr_augment_plan(a["B"], a["st"], a["p"], a["s"], a["mr"], a["ma"], a["R"], a["A"], a["seed"], a["rank"], a["tb"], a["fl"],
                                   None) == -1, bad
        assert b"hupr_augment_plan" in L.hupr_last_error()
    assert L.hupr_launch_count() == n0
    torch.cuda.synchronize()
    assert not st.any() and not tb.any()


# ---- noise and masks -----------------------------------------------------------------------------------------------------------------------
APPLY_SHAPES = [(3, 5, 8, 12, 1, 0), (2, 32, 64, 64, 1, 0), (1, 2, 64, 64, 8, 0), (2, 3, 8, 7, 1, 1), (2, 3, 5, 7, 1, 0), (2, 1, 6, 5, 3, 1)]
SEED, RANK, STEP = 99, 2, 6


def _table(B, R, A, sigmas):
    """A hand-made plan: sample b has sigma sigmas[b] and bands that depend on b (the first sample's range band is empty)."""
    t = np.zeros((B, 8), dtype=np.int32)
    for b in range(B):
        t[b, aug.SIGMA] = np.float32(sigmas[b]).view(np.int32)
        t[b, aug.RANGE_LEN], t[b, aug.RANGE_START] = (0, 3) if b == 0 else (min(2 + b, R // 2), 1 + b)
        t[b, aug.HORI_LEN], t[b, aug.HORI_START] = min(3, A // 2), b
        t[b, aug.VERT_LEN], t[b, aug.VERT_START] = (0, 0) if b == 1 else (min(2, A // 2), A - 2 - b)
    return t


def _mask(table, sensor, shape):
    B, P, R, A, E = shape
    m = np.zeros(shape, dtype=bool)
    ln, st = (aug.HORI_LEN, aug.HORI_START) if sensor == 0 else (aug.VERT_LEN, aug.VERT_START)
    for b in range(B):
        m[b, :, table[b, aug.RANGE_START]:table[b, aug.RANGE_START] + table[b, aug.RANGE_LEN]] = True
        m[b, :, :, table[b, st]:table[b, st] + table[b, ln]] = True
    return m


def _apply(x, y, shape, table, sensor):
    rt = _rt()
    B, P, R, A, E = shape
    state = torch.tensor([STEP + 1, 0, 0, 0], dtype=torch.int64, device=_dev())     # the plan drawn last was drawn at STEP
    rt.check(rt.lib().hupr_augment_apply_f32(x.data_ptr(), y.data_ptr(), B, P, R, A, E, rt.ptr(table), sensor, rt.ptr(state), SEED, RANK,
                                             rt.stream()))
    return y


def _input(shape, offset):
    n = int(np.prod(shape))
    x = synth.normal((n,), "augment_x", n).astype(np.float32)
    x[::17] = -0.0
    x[5::29] = np.nan
    buf = torch.zeros(n + 4, dtype=torch.float32, device=_dev())
    view = buf[offset:offset + n]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 * offset
    return x.reshape(shape), view


@pytest.mark.parametrize("B,P,R,A,E,offset", APPLY_SHAPES)
@pytest.mark.parametrize("sensor", [0, 1])
def test_masks_alone_zero_their_cells_and_keep_every_other_bit(B, P, R, A, E, offset, sensor):
    shape = (B, P, R, A, E)
    x, xd = _input(shape, offset)
    table = _table(B, R, A, [0.0] * B)
    out_buf = torch.full((x.size + 4,), 3.0, dtype=torch.float32, device=_dev())
    y = _apply(xd, out_buf[offset:offset + x.size], shape, torch.from_numpy(table).to(_dev()), sensor)
    got = y.cpu().numpy().reshape(shape)
    m = _mask(table, sensor, shape)
    assert m.any() and not m.all()
    assert (got[m].view(np.int32) == 0).all()                                       # exactly +0.0, NaN inputs included
    assert np.array_equal(got[~m].view(np.int32), x[~m].view(np.int32))
    assert np.array_equal(xd.cpu().numpy().view(np.int32), x.reshape(-1).view(np.int32))       # out of place: the input is untouched
    assert bool((out_buf[:offset] == 3.0).all()) and bool((out_buf[offset + x.size:] == 3.0).all())


@pytest.mark.parametrize("B,P,R,A,E,offset", APPLY_SHAPES)
def test_noise_against_fp64_box_muller_of_the_host_philox_words(B, P, R, A, E, offset):
    """|out - (x + sigma z64)| <= sigma 2e-6 (1 + |z|) + 2^-23 |out|: 2 ulp each for the logarithm and sinpif / cospif, carried through
    the square root and the product, plus one rounding of the fused multiply-add."""
    shape = (B, P, R, A, E)
    n = P * R * A * E
    x, xd = _input(shape, offset)
    x = np.nan_to_num(x, nan=0.25)
    xd.copy_(torch.from_numpy(x.reshape(-1)))
    sigmas = [0.5, 0.0, 1.25][:B] if B > 1 else [0.75]
    worst = 0.0
    for sensor in (0, 1):
        table = _table(B, R, A, sigmas)
        td = torch.from_numpy(table).to(_dev())
        y1 = _apply(xd, torch.empty_like(xd), shape, td, sensor)
        y2 = _apply(xd, torch.empty_like(xd), shape, td, sensor)
        assert torch.equal(_bits(y1), _bits(y2))                                    # two runs, equal bits
        inplace = xd.clone()
        _apply(inplace, inplace, shape, td, sensor)
        assert torch.equal(_bits(inplace), _bits(y1))
        got = y1.cpu().numpy().reshape(shape).astype(np.float64)
        m = _mask(table, sensor, shape)
        assert (got[m] == 0).all()
        for b in range(B):
            z = aug.noise_reference(STEP, SEED, RANK, sensor, b, n).reshape(shape[1:])
            sig = float(np.float32(sigmas[b]))
            want = x[b].astype(np.float64) + sig * z
            err = np.abs(got[b] - want)
            bound = sig * 2e-6 * (1 + np.abs(z)) + 2.0 ** -23 * np.abs(got[b])
            keep = ~m[b]
            worst = max(worst, float((err[keep] / np.maximum(bound[keep], 1e-300)).max()) if sig else 0.0)
            assert (err[keep] <= bound[keep]).all(), (b, sensor, float((err[keep] - bound[keep]).max()))
            if sig == 0.0:
                assert np.array_equal(y1.cpu().numpy().reshape(shape)[b][keep].view(np.int32), x[b][keep].view(np.int32))
    print("noise vs fp64 Box-Muller, shape %r: worst error / bound %.3f" % (shape, worst))
    # the horizontal and the vertical tensor draw from different domains
    t0 = torch.from_numpy(_table(B, R, A, [1.0] * B)).to(_dev())
    t0[:, 2:] = 0
    assert not torch.equal(_apply(xd, torch.empty_like(xd), shape, t0, 0), _apply(xd, torch.empty_like(xd), shape, t0, 1))


def test_the_four_byte_path_gives_the_vector_path_its_bits():
    shape = (2, 3, 8, 12, 1)
    x, aligned = _input(shape, 0)
    _, shifted = _input(shape, 1)
    td = torch.from_numpy(_table(2, 8, 12, [0.5, 2.0])).to(_dev())
    a = _apply(aligned, torch.empty_like(aligned), shape, td, 0)
    out_buf = torch.empty(x.size + 4, dtype=torch.float32, device=_dev())
    b = _apply(shifted, out_buf[1:1 + x.size], shape, td, 0)
    assert torch.equal(_bits(a), _bits(b))


def test_noise_statistics_at_sigma_one():
    shape = (2, 32, 64, 64, 1)
    n = 32 * 64 * 64
    x = torch.zeros(2 * n, dtype=torch.float32, device=_dev())
    t = np.zeros((2, 8), dtype=np.int32)
    t[:, aug.SIGMA] = np.float32(1.0).view(np.int32)
    z = _apply(x, torch.empty_like(x), shape, torch.from_numpy(t).to(_dev()), 0).cpu().numpy().astype(np.float64).reshape(2, n)
    assert np.isfinite(z).all() and not np.array_equal(z[0], z[1])
    # five standard errors of the mean and of the variance of n standard normal values: per sample (n = 131 072) and over the
    # tensor's 262 144 values
    for name, v in (("sample 0", z[0]), ("sample 1", z[1]), ("both samples", z.reshape(-1))):
        mean, var, k = v.mean(), v.var(), v.size
        print("%s: mean %.5f (bound %.5f), var - 1 %.5f (bound %.5f)" % (name, mean, 5 / np.sqrt(k), var - 1, 5 * np.sqrt(2 / k)))
        assert abs(mean) <= 5 / np.sqrt(k) and abs(var - 1) <= 5 * np.sqrt(2 / k)


def test_apply_argument_errors_launch_nothing():
    rt = _rt()
    L = rt.lib()
    x = torch.ones(2 * 3 * 8 * 8 + 4, dtype=torch.float32, device=_dev())
    tb = torch.zeros((2, 8), dtype=torch.int32, device=_dev())
    st = torch.ones(4, dtype=torch.int64, device=_dev())
    ok = dict(x=x.data_ptr(), y=x.data_ptr(), B=2, P=3, R=8, A=8, E=1, tb=tb.data_ptr(), sensor=0, st=st.data_ptr(), rank=0)
    n0 = L.hupr_launch_count()
    for bad in (dict(x=None), dict(y=None), dict(tb=None), dict(st=None), dict(B=0), dict(B=65536), dict(P=0), dict(R=0), dict(A=0), dict(E=0),
                dict(sensor=2), dict(sensor=-1), dict(rank=-1), dict(y=x.data_ptr() + 8), dict(x=x.data_ptr() + 2), dict(st=st.data_ptr() + 4),
                dict(P=1 << 30, R=1 << 16, A=1 << 16)):
        a = dict(ok, **bad)
        assert L.hupr_augment_apply_f32(a["x"], a["y"], a["B"], a["P"], a["R"], a["A"], a["E"], a["tb"], a["sensor"], a["st"], 1, a["rank"],
                                        None) == -1, bad
        assert b"hupr_augment_apply_f32" in L.hupr_last_error()
    assert L.hupr_launch_count() == n0
    torch.cuda.synchronize()
    assert bool((x == 1).all())


# ---- the labels ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def joints():
    """(4, 14, 2) int64 joints off the .5 tie (x / 4 is never on .5) and float joints with 1/64-pixel fractions, also off the tie."""
    j = synth.keypoints(4, 32).astype(np.int64)
    j[..., 0] += (j[..., 0] % 4 == 2)
    frac = synth.randint((4, 14, 2), 0, 64, "augment_frac", 1).astype(np.float32) / 64
    f = j.astype(np.float32) + frac
    tie = np.mod(f[..., 0], 4) == 2
    f[..., 0] += tie * 0.25
    return j, f


@pytest.mark.parametrize("kind", ["int64", "float32"])
def test_labels_against_torch(joints, kind):
    j = torch.from_numpy(joints[0] if kind == "int64" else joints[1]).to(_dev())
    j[0, 3, 0] = 255                                                                # beyond the axis: goes negative, stays a number
    keep = j.clone()
    flags = torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device=_dev())
    out = aug.mirror_joints(j, PAIRS, 252, flags)
    want = j.clone()
    sel = flags.bool()
    want[sel] = aug.mirror_joints_host(j[sel], PAIRS, 252)
    assert out.dtype == j.dtype and torch.equal(out, want) and torch.equal(j, keep)
    assert out[0, PAIRS[3], 0].item() == -3
    assert torch.equal(out[1], j[1]) and torch.equal(out[0, :, 1], j[0, PAIRS, 1])
    every = aug.mirror_joints(j, PAIRS, 252)
    assert torch.equal(every, aug.mirror_joints_host(j, PAIRS, 252))
    assert torch.equal(aug.mirror_joints(every, PAIRS, 252), j)                     # an involution
    rt = _rt()
    L = rt.lib()
    pair = (ctypes.c_int * 14)(*PAIRS)
    n0 = L.hupr_launch_count()
    o = torch.empty_like(j)
    for args in ((None, o.data_ptr(), 4, 14, pair), (j.data_ptr(), None, 4, 14, pair), (j.data_ptr(), j.data_ptr(), 4, 14, pair),
                 (j.data_ptr(), o.data_ptr(), -1, 14, pair), (j.data_ptr(), o.data_ptr(), 4, 65, pair), (j.data_ptr(), o.data_ptr(), 4, 0, pair),
                 (j.data_ptr(), o.data_ptr(), 4, 14, None), (j.data_ptr(), o.data_ptr(), 4, 14, (ctypes.c_int * 14)(*([1] * 14))),
                 (j.data_ptr(), o.data_ptr(), 4, 14, (ctypes.c_int * 14)(*([14] + PAIRS[1:])))):
        assert L.hupr_augment_joints(args[0], args[1], args[2], args[3], int(kind == "float32"), None, args[4], 252, None) == -1, args
    assert L.hupr_augment_joints(j.data_ptr(), o.data_ptr(), 4, 14, 2, None, pair, 252, None) == -1
    assert L.hupr_augment_joints(j.data_ptr(), o.data_ptr(), 4, 14, 0, None, pair, -1, None) == -1
    assert L.hupr_launch_count() == n0
    with pytest.raises(ValueError):
        aug.mirror_joints(j.to(torch.int32), PAIRS, 252)


def test_target_of_a_mirrored_label_is_the_mirror_of_the_target(joints):
    """With the axis at the centre of the heat-map grid the mirrored, left/right-exchanged target is the target of the mirrored label:
    to the rounding of expf for sub-pixel targets, bit for bit for integer targets off the .5 tie (tools/augment.py)."""
    from hupr_amd import functional as F_
    ji, jf = (torch.from_numpy(a).to(_dev()) for a in joints)
    t_sub = F_.gaussian_targets_subpixel(jf)
    t_sub_m = F_.gaussian_targets_subpixel(aug.mirror_joints(jf, PAIRS, 252))
    err = (t_sub_m - t_sub[:, PAIRS].flip(-1)).abs().max().item()
    print("sub-pixel targets: mirrored label vs mirrored target, max |diff| %.3e" % err)
    assert err <= 1e-6 and t_sub.max().item() > 0.9
    t_int = F_.gaussian_targets(ji)
    t_int_m = F_.gaussian_targets(aug.mirror_joints(ji, PAIRS, 252))
    assert torch.equal(_bits(t_int_m), _bits(t_int[:, PAIRS].flip(-1)))
    # the documented tie: x / 4 on .5 rounds up on both sides, the mirrored target is one pixel off
    tie = torch.tensor([[[102, 80]]], dtype=torch.int64, device=_dev())
    a = F_.gaussian_targets(aug.mirror_joints(tie, [0], 252))[0, 0].flatten().argmax().item() % 64
    b = F_.gaussian_targets(tie)[0, 0].flip(-1).flatten().argmax().item() % 64
    assert abs(a - b) == 1


# ---- the flip-test merge ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,offset", [((2, 14, 64, 64), 0), ((3, 14, 5, 7), 0), ((2, 14, 8, 8), 1)])
def test_merge_equals_the_torch_expression(shape, offset):
    n = int(np.prod(shape))
    bufs = [torch.zeros(n + 4, dtype=torch.float32, device=_dev()) for _ in range(2)]
    p, pm = (b[offset:offset + n].view(shape) for b in bufs)
    p.copy_(torch.from_numpy(synth.uniform(shape, 0.0, 1.0, "merge_p", n)))
    pm.copy_(torch.from_numpy(synth.uniform(shape, 0.0, 1.0, "merge_pm", n)))
    keep = (p.clone(), pm.clone())
    out = aug.flip_merge(p, pm, PAIRS)
    assert out.shape == p.shape and torch.equal(_bits(out), _bits(0.5 * (p + pm[:, PAIRS].flip(-1))))
    assert torch.equal(p, keep[0]) and torch.equal(pm, keep[1])
    # the merge commutes with the mirror: merge(p, pm) mirrored and exchanged is merge(pm, p), because the fp32 add commutes
    assert torch.equal(_bits(out[:, PAIRS].flip(-1)), _bits(aug.flip_merge(pm, p, PAIRS)))
    # the heads' own layouts: (B, K, 1, H, W) and (B, 1, K, H, W)
    assert torch.equal(aug.flip_merge(p.unsqueeze(2), pm.unsqueeze(2), PAIRS), out.unsqueeze(2))
    assert torch.equal(aug.flip_merge(p.unsqueeze(1), pm.unsqueeze(1), PAIRS), out.unsqueeze(1))


def test_merge_argument_errors_launch_nothing():
    rt = _rt()
    L = rt.lib()
    p = torch.ones((1, 14, 8, 8), dtype=torch.float32, device=_dev())
    o = torch.zeros_like(p)
    pair = (ctypes.c_int * 14)(*PAIRS)
    n0 = L.hupr_launch_count()
    for args in ((None, p.data_ptr(), o.data_ptr(), 1, 14, 8, 8, pair), (p.data_ptr(), None, o.data_ptr(), 1, 14, 8, 8, pair),
                 (p.data_ptr(), p.data_ptr(), None, 1, 14, 8, 8, pair), (p.data_ptr(), p.data_ptr(), p.data_ptr(), 1, 14, 8, 8, pair),
                 (p.data_ptr(), o.data_ptr(), o.data_ptr(), 1, 14, 8, 8, pair), (p.data_ptr(), p.data_ptr(), o.data_ptr(), -1, 14, 8, 8, pair),
                 (p.data_ptr(), p.data_ptr(), o.data_ptr(), 1, 14, 0, 8, pair), (p.data_ptr(), p.data_ptr(), o.data_ptr(), 1, 14, 8, 4097, pair),
                 (p.data_ptr(), p.data_ptr(), o.data_ptr(), 1, 14, 8, 8, None),
                 (p.data_ptr(), p.data_ptr(), o.data_ptr(), 1, 14, 8, 8, (ctypes.c_int * 14)(*([1, 2, 0] + list(range(3, 14)))))):
        assert L.hupr_flip_merge_f32(*args, None) == -1, args
        assert b"hupr_flip_merge_f32" in L.hupr_last_error()
    assert L.hupr_launch_count() == n0
    torch.cuda.synchronize()
    assert not o.any()
    with pytest.raises(ValueError):
        aug.flip_merge(p, p[:, :7], PAIRS)


# ---- the engine (B = 4, bf16; the sizes and bounds of tests/test_coord_loss_gpu.py's replay test) -----------------------------------------
@pytest.fixture(scope="module")
def batch():
    B = 4
    host_h = synth.adc_cube_int16(31, sensor=0, nframes=B * G)
    adc_h = torch.from_numpy(host_h).to(_dev())
    adc_hm = torch.from_numpy(aug.mirror_adc_host(host_h)).to(_dev())
    adc_v = torch.from_numpy(synth.adc_cube_int16(31, sensor=1, nframes=B * G)).to(_dev())
    return adc_h, adc_hm, adc_v, torch.from_numpy(synth.keypoints(B, 32)).to(_dev())


@pytest.fixture()
def bf16():
    from hupr_amd import functional as F_
    F_.set_math("bf16")
    yield F_
    F_.set_math("f32")


def test_a_mirrored_step_is_the_plain_step_on_the_host_permuted_cube(batch, bf16):
    from hupr_amd.tools.engine import TrainEngine
    adc_h, adc_hm, adc_v, joints = batch
    e1 = TrainEngine(_cfg(augMirror=1.0), device=_dev(), seed=0)
    e2 = TrainEngine(_cfg(), device=_dev(), seed=0)
    keep = adc_h.clone()
    l1, l1b = e1.train_step_from_adc(adc_h, adc_v, joints)
    l2, l2b = e2.train_step_from_adc(adc_hm, adc_v, aug.mirror_joints_host(joints, PAIRS, 252))
    torch.cuda.synchronize()
    print("mirrored step: loss %.6f vs %.6f" % (float(l1.detach()), float(l2.detach())))
    assert torch.equal(_bits(l1.detach().reshape(1)), _bits(l2.detach().reshape(1)))
    assert torch.equal(_bits(l1b.detach().reshape(1)), _bits(l2b.detach().reshape(1)))
    assert torch.equal(adc_h, keep)
    st = e1.augment_stats()
    assert st["steps"] == 1 and st["samples"] == 4 and st["mirrored"] == 4 and st["mean_sigma"] == 0.0
    assert e2.augment_stats() is None
    e1.close()
    e2.close()


def test_graph_replay_matches_eager_steps_with_augmentation(batch, bf16):
    """Five eager steps against 2 eager + capture (1 warm-up step) + 2 replays with all four keys set: the plan is drawn inside the
    step from the device counter, so the replays draw the plans of steps four and five."""
    from hupr_amd.tools.engine import TrainEngine
    adc_h, _, adc_v, joints = batch
    cfg = _cfg(**SETTINGS)
    e1 = TrainEngine(cfg, device=_dev(), seed=0)
    for _ in range(5):
        l1, _ = e1.train_step_from_adc(adc_h, adc_v, joints)
    e2 = TrainEngine(cfg, device=_dev(), seed=0)
    for _ in range(2):
        e2.train_step_from_adc(adc_h, adc_v, joints)
    e2.capture(adc_h, adc_v, joints, warmup=1)
    for _ in range(2):
        l2, _ = e2.train_step_from_adc(adc_h, adc_v, joints)
    torch.cuda.synchronize()
    s1, s2 = e1.augment_stats(), e2.augment_stats()
    p1 = torch.cat([p.detach().flatten() for p in e1.model.parameters()])
    p2 = torch.cat([p.detach().flatten() for p in e2.model.parameters()])
    rel = ((p1 - p2).norm() / p1.norm()).item()
    print("after 5 steps: parameters rel %.3e, loss %.6f vs %.6f, stats %s" % (rel, float(l1.detach()), float(l2.detach()),
                                                                               {k: v for k, v in s2.items() if k != "last_plan"}))
    assert np.array_equal(s1["last_plan"], s2["last_plan"])
    want, _ = aug.plan_reference(4, 4, 0, 0, 0.5, 0.75, 12, 20, 64, 64)
    assert np.array_equal(s1["last_plan"][:, [0, 2, 3, 4, 5, 6, 7]], want[:, [0, 2, 3, 4, 5, 6, 7]])
    for k in ("steps", "samples", "mirrored", "mean_sigma"):
        assert s1[k] == s2[k], k
    assert s1["steps"] == 5 and s1["samples"] == 20 and 0 < s1["mirrored"] < 20 and 0 < s1["mean_sigma"] < 0.75
    assert torch.isfinite(p2).all()
    assert rel <= 1e-5, rel
    assert abs(float(l1.detach()) - float(l2.detach())) <= 1e-4 * abs(float(l1.detach()))
    e1.close()
    e2.close()


def test_without_the_keys_nothing_is_launched_and_with_them_five_launches_more(batch, bf16):
    from hupr_amd.tools.engine import TrainEngine
    adc_h, _, adc_v, joints = batch
    L = _rt().lib()

    def count(fn):
        torch.cuda.synchronize()
        n0 = L.hupr_launch_count()
        fn()
        return L.hupr_launch_count() - n0

    e = TrainEngine(_cfg(), device=_dev(), seed=0)
    assert e.augment is None and e.augment_stats() is None
    e.train_step_from_adc(adc_h, adc_v, joints)                                     # the first step fills the host-side caches
    plain = count(lambda: e.train_step(*e.preprocess(adc_h, adc_v), joints))
    assert count(lambda: e.train_step_from_adc(adc_h, adc_v, joints)) == plain
    e.close()
    e = TrainEngine(_cfg(**SETTINGS), device=_dev(), seed=0)
    e.train_step_from_adc(adc_h, adc_v, joints)
    assert count(lambda: e.train_step_from_adc(adc_h, adc_v, joints)) == plain + 5  # plan, ADC mirror, two inputs, labels
    # micro-batches draw a plan each
    n = e.augment_stats()["steps"]
    e.train_step_accumulated([(adc_h[:2 * G], adc_v[:2 * G], joints[:2]), (adc_h[2 * G:], adc_v[2 * G:], joints[2:])])
    assert e.augment_stats()["steps"] == n + 2 and e.augment_stats()["last_plan"].shape == (2, 8)
    e.close()


def test_prenormalised_inputs_take_noise_and_masks_but_not_the_mirror(batch, bf16):
    from hupr_amd.tools.engine import TrainEngine
    adc_h, _, adc_v, joints = batch
    e = TrainEngine(_cfg(augMirror=0.5, augNoise=0.5), device=_dev(), seed=0)
    h, v = e.preprocess(adc_h, adc_v)
    with pytest.raises(RuntimeError, match="augMirror needs raw ADC cubes"):
        e.train_step(h, v, joints)
    assert e.augment_stats()["steps"] == 0
    e.close()
    e = TrainEngine(_cfg(augNoise=0.5, augMaskRange=8), device=_dev(), seed=0)
    h, v = e.preprocess(adc_h, adc_v)
    keep = (h.clone(), v.clone())
    loss, _ = e.train_step(h, v, joints)
    assert torch.isfinite(loss.detach()).item()
    assert torch.equal(h, keep[0]) and torch.equal(v, keep[1])                      # the caller's tensors are not written
    st = e.augment_stats()
    assert st["steps"] == 1 and st["mirrored"] == 0 and st["mean_sigma"] > 0
    # evaluation and infer never augment
    a = e.infer(h, v)
    b = e.infer(h, v)
    assert torch.equal(a[1], b[1]) and e.augment_stats()["steps"] == 1
    e.close()


# ---- the flip test ---------------------------------------------------------------------------------------------------------------------------
def test_flip_inference(batch, bf16):
    from hupr_amd.tools.engine import TrainEngine
    adc_h, adc_hm, adc_v, _ = batch
    adc_h, adc_hm, adc_v = adc_h[:2 * G], adc_hm[:2 * G], adc_v[:2 * G]
    e = TrainEngine(_cfg(augMirror=0.5), device=_dev(), seed=0)
    plain = e.infer_from_adc(adc_h, adc_v)
    again = e.infer_from_adc(adc_h, adc_v, flip=False)
    plain_m = e.infer_from_adc(adc_hm, adc_v)
    flipped = e.infer_from_adc(adc_h, adc_v, flip=True)
    flipped_m = e.infer_from_adc(adc_hm, adc_v, flip=True)
    assert e.augment_stats()["steps"] == 0                                          # inference never augments
    for h in range(2):
        assert torch.equal(_bits(plain[h]), _bits(again[h])) and flipped[h].shape == plain[h].shape
        assert torch.equal(_bits(flipped[h]), _bits(aug.flip_merge(plain[h], plain_m[h], PAIRS)))
        K, H, W = 14, plain[h].shape[-2], plain[h].shape[-1]
        a, b = flipped[h].reshape(-1, K, H, W), flipped_m[h].reshape(-1, K, H, W)
        assert torch.equal(_bits(b), _bits(a[:, PAIRS].flip(-1)))
        assert not torch.equal(plain[h], plain_m[h])
    e.close()


def _run_main(tmp_path, monkeypatch, name, test=None, **training):
    import yaml
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR
    cfgd = yaml.safe_load(open(os.path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"]["dataDir"] = "synthetic"
    cfgd["TRAINING"].update(batchSize=2, epochs=1, **training)
    cfgd["TEST"].update(batchSize=2, **(test or {}))
    for d in ("config", "logs", "visualization"):
        (tmp_path / d).mkdir(exist_ok=True)
    yaml.safe_dump(cfgd, open(tmp_path / "config" / (name + ".yaml"), "w"))
    monkeypatch.chdir(tmp_path)
    hmain.main(["--config", name + ".yaml", "--dir", name, "--synthetic_length", "4", "--max_steps", "2"])
    return tmp_path / "logs" / name


def test_runner_with_augmentation_and_the_flip_test(tmp_path, monkeypatch, capsys):
    run = _run_main(tmp_path, monkeypatch, "aug", test={"flip": True}, **SETTINGS)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("==========>Augmentation in epoch 0:")]
    assert len(lines) == 1 and "of 4 samples mirrored" in lines[0] and "(2 steps)" in lines[0]
    assert "AP: " in out and len([l for l in out.splitlines() if l.startswith("MPJPE: ")]) == 1
    ck = torch.load(run / "checkpoint.pth")
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "accuracy", "augment_step"} and ck["augment_step"] == 2
    # a resumed run goes on from the saved counter: the checkpoint's epoch is 0, so epoch 0 runs again, on the plans of steps 2 and 3
    from hupr_amd import main as hmain
    hmain.main(["--config", "aug.yaml", "--dir", "aug", "--synthetic_length", "4", "--max_steps", "2"])
    assert "==========>Load the augmentation counter (2 plans drawn)" in capsys.readouterr().out
    assert torch.load(run / "checkpoint.pth")["augment_step"] == 4
