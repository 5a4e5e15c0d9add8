"""The variable-Q transform without a GPU.  The longdouble restatement of its stages (tests/vqt_oracle.py) is held to what
the reference produced (tests/golden/vqt/cases.npz, made by tools/gen_golden_vqt.py) within 1e-12 of the largest
magnitude -- the margin is for the reference's FFT convolution; a float64 model of the same direct sums differs from it
by 5e-16 to 1.2e-15 -- and its resampler to scipy.signal.resample_poly within the forward bound of scipy's own float64
sums.  Then the new names, and every guard of the Python layer, all of which answer before the library is touched."""

import os

import numpy as np
import pytest
from scipy.signal import resample_poly

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend, transforms
from dsptoolbox_amd._lib import SIGNATURES, load_library
import vqt_cases as vc
import vqt_oracle

_cache = {}


def golden():
    if not _cache:
        z = np.load(vc.PATH, allow_pickle=False)
        _cache.update({k: z[k] for k in z.files})
    return _cache


def stored(name, full):
    """the part of a whole (F, N, C) result that the fixture stores"""
    if vc.stored_whole(name):
        return full
    rows, samples = vc.subset(name)
    return full[np.ix_(rows, samples)]


def test_new_names_exist():
    assert "vqt" in transforms.__all__ and callable(transforms.vqt) and "vqt" in transforms.__doc__
    assert callable(backend.vqt) and callable(backend.resample_int)
    header = open(os.path.join(vc.ROOT, "include", "dsptoolbox_amd.h")).read()
    lib = load_library()
    for name, n_args in (("ds_vqt", 16), ("ds_resample_int", 8)):
        assert f"int {name}(" in header and hasattr(lib, name)
        assert len(SIGNATURES[name][1]) == n_args
        declared = header.split(f"int {name}(")[1].split(");")[0]
        assert declared.count(",") + 1 == n_args


@pytest.mark.parametrize("name", list(vc.CASES))
def test_signals_are_rebuilt(name):
    x = vc.signal(name)
    assert np.array_equal(golden()[name + "_probe"], np.concatenate([x[:16, 0], [x.sum()]]))


@pytest.mark.parametrize("name", list(vc.CASES))
def test_oracle_reproduces_the_reference(name, capsys):
    z = golden()
    f, value, _, _ = vc.expected(name)
    assert np.array_equal(f, z[name + "_f"])
    ref = z[name + "_vqt"]
    mine = stored(name, value).astype(np.complex128)
    assert mine.shape == ref.shape
    scale = float(z[name + "_max"])
    worst = float(np.abs(mine - ref).max() / scale)
    with capsys.disabled():
        print(f"\n{name}: worst |oracle - reference| / max|reference| = {worst:.3g}")
    assert worst <= 1e-12


def test_subset_holds_the_rows_and_samples_asked_for():
    for name in vc.CASES:
        if vc.stored_whole(name):
            continue
        rows, samples = vc.subset(name)
        p = vc.CASES[name]
        bins = p["kw"].get("bins_per_octave", 24)
        for o in range(vc.n_rows(name) // bins):
            assert {o * bins, o * bins + bins // 2, o * bins + bins - 1} <= set(rows.tolist())
        assert set(range(64)) | set(range(p["n"] - 64, p["n"])) <= set(samples.tolist())


@pytest.mark.parametrize("up,down", vc.RATIOS)
@pytest.mark.parametrize("n", vc.RATIO_LENGTHS)
@pytest.mark.parametrize("complex_", [False, True])
def test_oracle_resampler_is_scipys(up, down, n, complex_, capsys):
    x = vc.ratio_signal(n, complex_)
    want = resample_poly(x, up, down, axis=0)
    y, a = vqt_oracle.resample_poly(x, up, down)
    assert y.shape == want.shape
    terms = 1 if max(up, down) == 1 else 20 * max(up, down) + 1  # scipy sums every tap, zeros included
    err = np.abs(y - want).astype(np.float64)
    lim = vqt_oracle.bound(a, terms + 2)
    worst = float((err / np.where(lim > 0, lim, 1.0)).max())
    with capsys.disabled():
        print(f"\nP({up}, {down}) n = {n} {'complex' if complex_ else 'real'}: worst |oracle - scipy| / bound = {worst:.3g}")
    assert (err <= lim).all()


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(backend, "get_context", refuse)
    monkeypatch.setattr(backend, "load_library", refuse)


def _signal(n, c, fs):
    return dsp.Signal(None, np.random.default_rng(5).standard_normal((n, c)), fs)


def test_channel_subset_is_the_references_value_error(no_library):
    with pytest.raises(ValueError, match="along dimension 2"):
        transforms.vqt(_signal(400, 2, 48000), channel=0)
    with pytest.raises(ValueError, match="along dimension 2"):
        transforms.vqt(_signal(400, 3, 48000), channel=np.array([0, 2]))


def test_top_octave_above_nyquist_divides_by_zero(no_library):
    with pytest.raises(ZeroDivisionError):
        transforms.vqt(_signal(400, 1, 8000), octaves=[4, 7])  # highest_f = 3951 Hz: d = 0


def test_bounds_are_named(no_library):
    with pytest.raises(NotImplementedError, match="VQT_MAX_DECIMATION = 48"):
        transforms.vqt(_signal(400, 1, 192000), octaves=[1, 4])  # d = 176
    with pytest.raises(NotImplementedError, match="VQT_MAX_OCTAVES = 7"):
        transforms.vqt(_signal(400, 1, 48000), octaves=[-2, 5])
    with pytest.raises(NotImplementedError, match="VQT_MAX_KERNEL = 2048"):
        transforms.vqt(_signal(400, 1, 48000), gamma=0, bins_per_octave=400)
    with pytest.raises(NotImplementedError, match="VQT_MAX_ROWS = 65535"):
        transforms.vqt(_signal(400, 1, 48000), bins_per_octave=14000, gamma=5000)
    with pytest.raises(NotImplementedError, match="VQT_MAX_OUTPUT_BYTES = 2\\^34"):
        backend._vqt_guard(1 << 23, 2, 22, 5, 24, 127)
    with pytest.raises(NotImplementedError, match="VQT_MAX_DECIMATION"):
        backend.resample_int(np.zeros((10, 1)), 1, 49)
    with pytest.raises(ValueError, match="one of up and down"):
        backend.resample_int(np.zeros((10, 1)), 3, 2)
    assert backend._vqt_interp_tile(3, 3) == vc.INTERP_TILE and backend._vqt_interp_tile(22, 2) == 2024 and backend.VQT_SAMPLE_TILE == {1: 256, 2: 128}
