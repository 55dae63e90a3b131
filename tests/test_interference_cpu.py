"""CPU (-m "not gpu"): the interference filter's settings, sidecar and refusals, and what its RULE does — on the numpy statement
(tests/interference_ref.py), through the oracle's FFT chain.  The device kernel is compared with the same statement bit for bit in
tests/test_interference_gpu.py."""
import numpy as np
import pytest

import interference_ref as R
from hupr_amd import synth
from hupr_amd.config_tree import load_config
from hupr_amd.preprocessing import InterferenceFilter, interference_setting
from hupr_amd.preprocessing import interference as itf
from hupr_amd.preprocessing import process_iwr1843 as pre
from hupr_amd.tools import augment as aug
from hupr_amd.tools import base as tools_base


def _cfg(**dataset):
    cfg = load_config()
    for k, v in dataset.items():
        setattr(cfg.DATASET, k, v)
    return cfg


class _Tree:
    """A YAML mapping the way config_tree hands it over: attributes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---- settings ---------------------------------------------------------------------------------------------------------------------------
def test_the_value_object():
    f = InterferenceFilter()
    assert (f.K, f.guard, f.fill) == (32, 2, "clutter") and repr(f) == "InterferenceFilter(K=32, guard=2, fill='clutter')"
    assert f == InterferenceFilter(32, 2, "clutter") and hash(f) == hash(InterferenceFilter(K=np.int64(32)))
    assert f != InterferenceFilter(K=16) and f != InterferenceFilter(fill="zero") and len({f, InterferenceFilter(), InterferenceFilter(guard=0)}) == 2
    with pytest.raises(AttributeError):
        f.K = 8
    with pytest.raises(AttributeError):
        del f.guard
    assert InterferenceFilter(2, 0, "zero").sidecar() == {"threshold": 2, "guard": 0, "fill": "zero"}
    InterferenceFilter(1024, 8)
    for kw in (dict(K=1), dict(K=1025), dict(K=32.0), dict(K=True), dict(K="32"), dict(guard=-1), dict(guard=9), dict(guard=2.0),
               dict(guard=False), dict(fill="mean"), dict(fill=None), dict(fill=0)):
        with pytest.raises(ValueError):
            InterferenceFilter(**kw)


def test_setting_parsing():
    assert interference_setting(_cfg()) is None                          # absent: off (the shipped config has no such key)
    assert interference_setting(_cfg(interference=False)) is None
    assert interference_setting(_cfg(interference=True)) == InterferenceFilter()
    assert interference_setting(_cfg(interference=_Tree(threshold=16))) == InterferenceFilter(K=16)
    assert interference_setting(_cfg(interference=_Tree(guard=0, fill="zero"))) == InterferenceFilter(guard=0, fill="zero")
    assert interference_setting(_cfg(interference={"threshold": 64, "guard": 4, "fill": "clutter"})) == InterferenceFilter(64, 4, "clutter")
    assert interference_setting(_cfg(interference=_Tree())) == InterferenceFilter()
    for bad in (1, 0, 32.0, "true", "clutter", [32, 2], _Tree(K=16), _Tree(threshold=16, pfa=1e-3), _Tree(threshold=1),
                _Tree(threshold=16.0), _Tree(guard=9), _Tree(fill="median"), {"threshold": True}):
        with pytest.raises(ValueError, match="DATASET.interference"):
            interference_setting(_cfg(interference=bad))


def test_the_sidecar_names_the_filter_only_when_it_is_on():
    off = tools_base.preprocess_sidecar(_cfg())
    assert off == {"fft_zero_doppler": pre.ZERO_DOPPLER}
    assert tools_base.preprocess_sidecar(_cfg(interference=False)) == off
    on = tools_base.preprocess_sidecar(_cfg(interference=True))
    assert on == dict(off, adc_interference={"threshold": 32, "guard": 2, "fill": "clutter"})
    assert tools_base.preprocess_sidecar(_cfg(interference=_Tree(threshold=8, fill="zero")))["adc_interference"] == \
        {"threshold": 8, "guard": 2, "fill": "zero"}
    # the mismatch warning: both ways and between two settings; a sidecar without the key means off
    f = InterferenceFilter()
    assert itf.interference_mismatch_warning(off, None) is None and itf.interference_mismatch_warning(on, f) is None
    assert "trained with DATASET.interference off" in itf.interference_mismatch_warning(off, f)
    assert "this process runs it off" in itf.interference_mismatch_warning(on, None)
    assert "'threshold': 16" in itf.interference_mismatch_warning(on, InterferenceFilter(K=16))


def test_stored_cube_dataset_refuses_the_key():
    from hupr_amd.datasets.dataset import HuPR3D_horivert
    with pytest.raises(RuntimeError, match="already filtered and are used with the key off"):
        HuPR3D_horivert("train", _cfg(interference=True), None)
    with pytest.raises(ValueError, match="DATASET.interference"):
        HuPR3D_horivert("train", _cfg(interference=7), None)


def test_the_stream_command_parses_the_filter():
    from hupr_amd.tools import stream as st
    assert st.interference_from_args(st.parse(["--raw", "x"])) is None
    assert st.interference_from_args(st.parse(["--raw", "x", "--interference"])) == InterferenceFilter()
    a = st.parse(["--raw", "x", "--interference", "--interference-threshold", "16", "--interference-guard", "0", "--interference-fill", "zero"])
    assert st.interference_from_args(a) == InterferenceFilter(16, 0, "zero")
    for argv in (["--interference-guard", "3"], ["--interference", "--interference-threshold", "1"], ["--interference", "--interference-guard", "9"]):
        with pytest.raises(SystemExit):
            st.parse(["--raw", "x"] + argv)
    assert issubclass(st.InterferenceError, st.StreamError)
    with pytest.raises(st.InterferenceError):
        st.check_interference({"threshold": 32})


# ---- the generator ----------------------------------------------------------------------------------------------------------------------
def test_interference_bursts():
    clean = R.clean_scene(0)
    cube, mask = synth.interference_bursts(clean, R.BURST_CHIRPS, amp=4000.0, length=(8, 24), seed=0)
    assert cube.dtype == np.int16 and cube.shape == clean.shape and mask.shape == clean.shape[:-1] and mask.dtype == bool
    changed = (cube != clean).any(axis=-1)
    assert not (changed & ~mask).any() and changed[mask].mean() > 0.99
    per_chirp = mask[0, 0].sum(axis=-1)
    assert sorted(np.flatnonzero(per_chirp)) == list(R.BURST_CHIRPS) and per_chirp[per_chirp > 0].min() >= 8 and per_chirp.max() <= 24
    assert (mask[0] == mask[0, :1]).all()                                         # all four receivers
    again, _ = synth.interference_bursts(clean, R.BURST_CHIRPS, amp=4000.0, length=(8, 24), seed=0)
    other, _ = synth.interference_bursts(clean, R.BURST_CHIRPS, amp=4000.0, length=(8, 24), seed=1)
    assert np.array_equal(again, cube) and not np.array_equal(other, cube)
    none, m0 = synth.interference_bursts(clean[0], [], seed=3)
    assert np.array_equal(none, clean[0]) and not m0.any() and m0.shape == (4, 192, 256)
    for bad in (dict(chirps=[192]), dict(chirps=[3, 3]), dict(chirps=[1], length=0), dict(chirps=[1], length=(9, 8))):
        with pytest.raises(ValueError):
            synth.interference_bursts(clean, **bad)
    with pytest.raises(ValueError):
        synth.interference_bursts(clean.astype(np.int32), [1])


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    cube, clean, injected = R.burst_scene(0)
    return cube, clean, injected, {fill: R.interference_ref(cube, 32, 2, fill) for fill in ("clutter", "zero")}


def test_a_clean_scene_passes_bit_for_bit(scene):
    _, clean, _, _ = scene
    for fill in ("clutter", "zero"):
        r = R.interference_ref(clean, 32, 2, fill)
        assert not r["flags"].any() and np.array_equal(r["cube"], clean) and not r["mask"].any() and not r["groups"].any() and not r["frames"].any()


def test_no_injected_sample_is_missed_and_every_extra_flag_is_guard(scene):
    cube, _, injected, refs = scene
    flags = refs["clutter"]["flags"]
    assert injected.sum() > 1000
    assert not (injected & ~flags).any()
    assert not (flags & ~R.dilate(injected, 2)).any()
    assert np.array_equal(flags, refs["zero"]["flags"])
    # a per-chirp threshold on the RAW envelope finds nothing: the static reflector sets the chirp's median
    x = cube.astype(np.int64)
    env = x[..., 0] ** 2 + x[..., 1] ** 2
    assert not (env > 32 * np.median(env, axis=-1, keepdims=True)).any()
    # counts and mask are the flags'
    r = refs["clutter"]
    assert r["frames"][0, 0] == flags.sum() and r["frames"][0, 1] == flags.any(axis=-1).sum() == 4 * len(R.BURST_CHIRPS)
    assert np.array_equal(np.unpackbits(r["mask"], axis=-1, bitorder="little").astype(bool), flags)
    assert np.array_equal(r["cube"][~flags], cube[~flags]) and (refs["zero"]["cube"][flags] == 0).all()


def test_through_the_oracle_chain_the_filter_removes_most_of_the_error(scene):
    from oracle import fft_chain as offt
    cube, clean, _, refs = scene

    def heat(iq):
        return offt.generate_heatmap(synth.adc_cube_complex(iq)[0])

    base = heat(clean)
    e_int, e_clutter, e_zero = (np.linalg.norm(heat(c) - base) / np.linalg.norm(base) for c in (cube, refs["clutter"]["cube"], refs["zero"]["cube"]))
    print("rel-L2 against the clean scene's cube: unfiltered %.4f  clutter fill %.4f  zero fill %.4f" % (e_int, e_clutter, e_zero))
    assert e_clutter < e_zero < e_int
    assert e_clutter < 0.5 * e_int


def test_noise_only_flag_rate_is_two_to_the_minus_k():
    noise = synth.point_target_cube([], noise=300.0, seed=11)
    rate = R.interference_ref(noise, 8, 0, "clutter")["flags"].mean()
    print("flag rate under noise at K = 8: %.3e = %.2f x 2^-8" % (rate, rate * 256))
    assert 0.5 * 2.0 ** -8 < rate < 2.0 * 2.0 ** -8


def test_the_filter_commutes_with_the_mirror(scene):
    cube, _, _, refs = scene
    for fill in ("clutter", "zero"):
        m = R.interference_ref(aug.mirror_adc_host(cube), 32, 2, fill)
        assert np.array_equal(m["cube"], aug.mirror_adc_host(refs[fill]["cube"]))
        assert np.array_equal(m["flags"], aug.mirror_adc_host(refs[fill]["flags"][..., None])[..., 0])
        assert np.array_equal(m["frames"], refs[fill]["frames"])
