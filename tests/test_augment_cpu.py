"""CPU (-m "not gpu"): the host half of the radar augmentation (hupr_amd/tools/augment.py) — the settings, the joint pair table, the
numpy Philox4x32-10 against its known-answer vectors, the host plan, and the identity that pins the ADC permutation to the FFT
chain's layout: the chain's output for the permuted cube is the azimuth index map (62 - a) mod 64 times a per-bin phase ramp of the
plain output."""
import numpy as np
import pytest

from hupr_amd import synth
from hupr_amd.config_tree import load_config
from hupr_amd.tools import augment as aug
from oracle import fft_chain as offt

SHIPPED_PAIRS = [3, 4, 5, 0, 1, 2, 6, 7, 11, 12, 13, 8, 9, 10]


def _cfg(test=None, **training):
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    for k, v in (test or {}).items():
        setattr(cfg.TEST, k, v)
    return cfg


# ---- settings ----------------------------------------------------------------------------------------------------------------------
def test_absent_keys_mean_no_augmentation():
    cfg = _cfg()
    assert aug.augment_settings(cfg) is None and aug.flip_setting(cfg) is False
    assert aug.augment_settings(_cfg(augMirror=-1, augNoise=-1, augMaskRange=-1, augMaskAngle=-1)) is None


def test_valid_settings():
    assert aug.augment_settings(_cfg(augMirror=0.5)) == {"p_mirror": 0.5, "sigma_max": 0, "max_range": 0, "max_angle": 0}
    assert aug.augment_settings(_cfg(augMirror=1, augNoise=0.25, augMaskRange=32, augMaskAngle=1)) == \
        {"p_mirror": 1.0, "sigma_max": 0.25, "max_range": 32, "max_angle": 1}
    assert aug.augment_settings(_cfg(augNoise=2)) == {"p_mirror": 0, "sigma_max": 2.0, "max_range": 0, "max_angle": 0}
    assert aug.flip_setting(_cfg(test={"flip": True})) is True and aug.flip_setting(_cfg(test={"flip": False})) is False


@pytest.mark.parametrize("key,value", [
    ("augMirror", 0), ("augMirror", 0.0), ("augMirror", 1.5), ("augMirror", -0.5), ("augMirror", float("nan")), ("augMirror", True),
    ("augMirror", "0.5"), ("augMirror", [0.5]), ("augMirror", None),
    ("augNoise", 0), ("augNoise", -2.0), ("augNoise", float("inf")), ("augNoise", float("nan")), ("augNoise", True), ("augNoise", "1"),
    ("augNoise", 1e39), ("augNoise", 1e-60), ("augNoise", None),
    ("augMaskRange", 0), ("augMaskRange", 33), ("augMaskRange", 4.0), ("augMaskRange", True), ("augMaskRange", -2), ("augMaskRange", "4"),
    ("augMaskAngle", 0), ("augMaskAngle", 33), ("augMaskAngle", 2.5), ("augMaskAngle", False), ("augMaskAngle", -3), ("augMaskAngle", [4]),
])
def test_invalid_training_settings_raise(key, value):
    with pytest.raises(ValueError, match="TRAINING." + key):
        aug.augment_settings(_cfg(**{key: value}))


@pytest.mark.parametrize("value", [0, 1, -1, "true", None, 1.0])
def test_invalid_flip_setting_raises(value):
    with pytest.raises(ValueError, match="TEST.flip"):
        aug.flip_setting(_cfg(test={"flip": value}))


def test_band_limits_follow_the_dataset_sizes():
    cfg = _cfg(augMaskRange=16)
    cfg.DATASET.rangeSize = 30
    with pytest.raises(ValueError, match="augMaskRange"):
        aug.augment_settings(cfg)
    cfg.DATASET.rangeSize = 32
    assert aug.augment_settings(cfg)["max_range"] == 16


# ---- pair table ----------------------------------------------------------------------------------------------------------------------
def test_pair_table_of_the_shipped_joint_list():
    pairs = aug.mirror_pairs(load_config().DATASET.idxToJoints)
    assert pairs == SHIPPED_PAIRS
    assert [pairs[p] for p in pairs] == list(range(14))


@pytest.mark.parametrize("names", [["L_Hip", "Neck"], ["Neck", "R_Knee", "L_Hip", "R_Hip"], ["Neck", "Neck"], ["L_Hip", "R_Hip", 3]])
def test_one_sided_or_repeated_names_raise(names):
    with pytest.raises(ValueError, match="mirror_pairs"):
        aug.mirror_pairs(names)


# ---- Philox ----------------------------------------------------------------------------------------------------------------------------
def _philox_by_the_book(ctr, key):
    """Philox4x32-10 written from the algorithm in plain Python integers."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_philox_known_answers():
    zero = aug.philox4x32([0, 0, 0, 0], [0, 0])
    ones = aug.philox4x32([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)
    assert zero.dtype == np.uint32
    assert [int(x) for x in zero] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(x) for x in ones] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert _philox_by_the_book([0] * 4, [0] * 2) == [int(x) for x in zero]


def test_philox_vectorised_equals_the_plain_integer_form():
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, size=(7, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(2,), dtype=np.uint64)
    got = aug.philox4x32(ctr, key)
    assert got.shape == (7, 4)
    for i in range(7):
        assert [int(x) for x in got[i]] == _philox_by_the_book([int(x) for x in ctr[i]], [int(x) for x in key])


# ---- the host plan -------------------------------------------------------------------------------------------------------------------
def test_plan_reference_follows_the_stated_rule():
    B, step, seed, rank = 5, (1 << 32) + 3, 11, 2
    table, flags = aug.plan_reference(B, step, seed, rank, 0.5, 0.75, 6, 9, 64, 48)
    assert table.shape == (B, 8) and table.dtype == np.int32 and flags.dtype == np.uint8
    sigma = aug.plan_sigma(table)
    for b in range(B):
        w0 = _philox_by_the_book([3, 1, b, 0], [seed, 4 * rank])
        w1 = _philox_by_the_book([3, 1, b, 1], [seed, 4 * rank])
        u = [(w >> 8) / 2.0 ** 24 for w in w0 + w1]
        rl = int(u[2] * 7)
        hl, vl = int(u[4] * 10), int(u[6] * 10)
        assert table[b, aug.MIRROR] == flags[b] == (u[0] < 0.5)
        assert abs(float(sigma[b]) - 0.75 * u[1]) <= 2.0 ** -24 * 0.75
        assert list(table[b, 2:]) == [rl, int(u[3] * (64 - rl + 1)), hl, int(u[5] * (48 - hl + 1)), vl, int(u[7] * (48 - vl + 1))]
    # bands stay inside the map; keys that are off draw nothing
    big, _ = aug.plan_reference(512, 0, 1, 0, 1.0, 0.0, 32, 32, 64, 64)
    assert big[:, aug.MIRROR].all() and not big[:, aug.SIGMA].any()
    for ln, st, size in ((aug.RANGE_LEN, aug.RANGE_START, 64), (aug.HORI_LEN, aug.HORI_START, 64), (aug.VERT_LEN, aug.VERT_START, 64)):
        assert big[:, ln].min() == 0 and big[:, ln].max() == 32 and (big[:, st] >= 0).all() and (big[:, st] + big[:, ln] <= size).all()
    off, flags = aug.plan_reference(64, 9, 1, 0, 0.0, 0.0, 0, 0, 64, 64)
    assert not off[:, [aug.MIRROR, aug.SIGMA, aug.RANGE_LEN, aug.HORI_LEN, aug.VERT_LEN]].any() and not flags.any()      # empty bands
    # the rank and the step are in the key and the counter
    a, _ = aug.plan_reference(8, 0, 1, 0, 0.5, 1.0, 8, 8, 64, 64)
    assert not np.array_equal(a, aug.plan_reference(8, 0, 1, 1, 0.5, 1.0, 8, 8, 64, 64)[0])
    assert not np.array_equal(a, aug.plan_reference(8, 1, 1, 0, 0.5, 1.0, 8, 8, 64, 64)[0])
    assert np.array_equal(a, aug.plan_reference(8, 0, 1, 0, 0.5, 1.0, 8, 8, 64, 64)[0])


def test_noise_reference_is_standard_normal():
    z = aug.noise_reference(4, 7, 0, 0, 1, 262143)
    n = z.size
    assert n == 262143 and np.isfinite(z).all()
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    assert not np.array_equal(z[:64], aug.noise_reference(4, 7, 0, 1, 1, 64))            # the sensor is in the key


# ---- the permutation against the FFT chain's layout --------------------------------------------------------------------------------------
def test_host_permutation_is_an_involution_and_moves_the_stated_rows():
    iq = synth.adc_cube_int16(31)
    m = aug.mirror_adc_host(iq)
    assert m.shape == iq.shape and m.dtype == np.int16 and not np.array_equal(m, iq)
    assert np.array_equal(aug.mirror_adc_host(m), iq)
    for rx, cc, tx in ((0, 0, 0), (1, 5, 1), (3, 63, 2), (2, 17, 0)):
        assert np.array_equal(m[0, rx, 3 * cc + tx], iq[0, 3 - rx, 3 * cc + (2 - tx)])


def test_chain_output_of_the_permuted_cube_is_index_map_times_ramp():
    iq = synth.adc_cube_int16(31)
    plain = offt.generate_heatmap(synth.adc_cube_complex(iq)[0])
    perm = offt.generate_heatmap(synth.adc_cube_complex(aug.mirror_adc_host(iq))[0])
    a = np.arange(64)
    ramp = np.exp(-2j * np.pi * 7 * ((31 - a) % 64) / 64)
    want = plain[:, :, (62 - a) % 64, :] * ramp[None, None, :, None]
    keep = np.arange(16) != 8
    rel = np.abs(perm[keep] - want[keep]).max() / np.abs(want[keep]).max()
    print("permuted cube vs index map x ramp: rel %.3e" % rel)
    assert rel <= 1e-12
    # the plain reversal of the azimuth axis is not it
    assert np.abs(np.abs(perm[keep]) - np.abs(plain[keep][:, :, ::-1, :])).max() > 0.05 * np.abs(plain[keep]).max()


def test_point_target_moves_from_bin_22_to_bin_40():
    iq = synth.point_target_cube([dict(range_bin=60, doppler_bin=3, az_bin=9, el_bin=0, amp=400.0)])

    def peak(cube):
        out = np.abs(offt.generate_heatmap(synth.adc_cube_complex(cube)[0]))
        return int(np.unravel_index(out.argmax(), out.shape)[2])
    assert peak(iq) == 22
    assert peak(aug.mirror_adc_host(iq)) == 40


def test_host_joint_mirror():
    j = np.array([[[10, 20], [30, 40], [250, 60]]], dtype=np.int64)
    out = aug.mirror_joints_host(j, [1, 0, 2], 252)
    assert out.tolist() == [[[222, 40], [242, 20], [2, 60]]]
