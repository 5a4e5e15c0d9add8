"""CleanSC, Orthogonal, Functional and MVDR beamformers (beamforming/beamforming.py:883-1314 of the reference) on
the device, float64 throughout.  tests/golden/beamformers/cases.npz is the reference's own output
(tools/gen_golden_beamformers.py): 16 microphones, three monopoles and sensor noise; PSD scaling (a positive
semi-definite CSM) and the default FFTBackward scaling (an indefinite one); a 1/3-octave band and a single bin."""

import numpy as np
import pytest
from scipy.integrate import simpson

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd.beamforming import (BeamformerCleanSC, BeamformerFunctional, BeamformerMVDR,
                                        BeamformerOrthogonal)
from dsptoolbox_amd.standard.enums import SpectrumScaling
from conftest import load_golden

TOL = 1e-6


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


class _Signal:  # what the constructors and argument checks read of a multi-channel Signal
    number_of_channels = 16


class _Grid:  # the reference's geometry classes stay the reference's: stand-ins with its interface
    def __init__(self, n, shape):
        self.number_of_points, self.shape = n, shape

    def reconstruct_map_shape(self, m):
        return np.asarray(m).reshape(self.shape)  # Regular2DGrid: a plain reshape of the flat map


class _Steering:
    def __init__(self, h):
        self.h = h

    def get_vector(self, wave_numbers, grid, mic):
        assert len(wave_numbers) == self.h.shape[0]  # the same bins as the reference selected
        return self.h


CLASSES = dict(mvdr=BeamformerMVDR, functional=BeamformerFunctional, orthogonal=BeamformerOrthogonal,
               cleansc=BeamformerCleanSC)


def _device_map(c, csm, h):
    kw = c["kwargs"]
    if c["method"] == "cleansc":
        return backend.beamformer_cleansc_map(csm, h, kw.get("maximum_iterations", 2 * csm.shape[1]),
                                              kw.get("safety_factor", 0.5), kw.get("remove_csm_diagonal", False))
    return backend.beamformer_eig_map(csm, h, c["method"], gamma=kw.get("gamma", 10),
                                      n_eig=kw.get("number_eigenvalues", csm.shape[1] // 2))


def _check(c, m, ref):
    e = relmax(m.ravel(), ref.ravel())
    assert e < TOL, (c, e)
    if c["method"] in ("orthogonal", "cleansc"):  # the sources land on the same grid points
        assert np.array_equal(np.flatnonzero(m.ravel()), np.flatnonzero(ref.ravel())), c
    return e


# ---- without a GPU: the interface ---------------------------------------------------------------
def test_beamformer_classes_exported():
    import dsptoolbox_amd.beamforming as bfm
    for name in ("BeamformerCleanSC", "BeamformerOrthogonal", "BeamformerFunctional", "BeamformerMVDR"):
        assert name in bfm.__all__ and hasattr(dsp.beamforming, name)


@pytest.mark.parametrize("cls", [BeamformerCleanSC, BeamformerOrthogonal, BeamformerFunctional, BeamformerMVDR])
def test_beamformer_constructor_checks(cls):
    bf = cls(_Signal(), None, _Grid(4, (2, 2)), _Steering(None), c=340)
    assert bf.c == 340 and bf.beamformer_type
    with pytest.raises(AssertionError):
        cls(_Signal(), None, _Grid(4, (2, 2)), _Steering(None), c=0)
    one = _Signal()
    one.number_of_channels = 1
    with pytest.raises(AssertionError):
        cls(one, None, _Grid(4, (2, 2)), _Steering(None))


def test_cleansc_rejects_invalid_arguments():
    bf = BeamformerCleanSC(_Signal(), None, _Grid(4, (2, 2)), _Steering(None))
    for kw in (dict(safety_factor=0.0), dict(safety_factor=1.5), dict(safety_factor=-0.1),
               dict(maximum_iterations=0), dict(maximum_iterations=-3)):
        with pytest.raises(AssertionError):
            bf.get_beamformer_map(1000.0, 3, **kw)


def test_orthogonal_rejects_invalid_arguments():
    bf = BeamformerOrthogonal(_Signal(), None, _Grid(4, (2, 2)), _Steering(None))
    for n in (0, -1, 17):
        with pytest.raises(AssertionError):
            bf.get_beamformer_map(1000.0, 3, number_eigenvalues=n)


# ---- on the device ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_beamformers_backend_golden():
    """Every fixture case from the stored CSM slice and steering vectors, integrated as the reference does."""
    meta, z = load_golden("beamformers/cases")
    worst = {}
    for i, c in enumerate(meta["cases"]):
        f, h, csm = z[f"f_{c['band']}"], z[f"h_{c['band']}"], z[f"csm_{c['scaling']}_{c['band']}"]
        m = _device_map(c, csm, h)
        assert m.shape == (h.shape[2], len(f))
        m = simpson(m, dx=f[1] - f[0], axis=1) if len(f) > 1 else m.squeeze()
        e = _check(c, m, z[f"map_{i}"])
        worst[c["method"]] = max(worst.get(c["method"], 0.0), e)
    print("worst relative max error per method:", worst)


@pytest.mark.gpu
def test_beamformers_classes_from_time_data_golden():
    """The classes end to end from the microphone signals: Signal.get_csm() (a short estimate: the float64 route),
    the band selection, the device map and the Simpson integration, against the reference's final maps."""
    meta, z = load_golden("beamformers/cases")
    for i, c in enumerate(meta["cases"]):
        s = dsp.Signal(None, z["time_data"].astype(np.float64), meta["fs"])
        s.set_spectrum_parameters(window_length_samples=meta["window"], scaling=SpectrumScaling[c["scaling"]])
        bf = CLASSES[c["method"]](s, None, _Grid(c["n_points"], c["grid_shape"]), _Steering(z[f"h_{c['band']}"]))
        m = bf.get_beamformer_map(c["center_hz"], c["octave_fraction"], **c["kwargs"])
        assert m.shape == tuple(c["grid_shape"])
        assert np.array_equal(bf.f_range_hz, z[f"f_{c['band']}"][[0, -1]])
        _check(c, m, z[f"map_{i}"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 16, 33, 64])
def test_hermitian_eigh_indefinite(n):
    rng = np.random.default_rng(100 + n)
    x = rng.standard_normal((3, n, n)) + 1j * rng.standard_normal((3, n, n))
    a = x + np.conj(np.swapaxes(x, 1, 2))
    a[1] *= 1e-3  # scale does not matter
    a[2] = a[2] @ a[2].conj().T  # a semi-definite one
    w, v = backend.hermitian_eigh(a)
    for k in range(3):
        na = np.linalg.norm(a[k], 2)
        assert np.all(np.diff(w[k]) >= 0)
        assert np.max(np.abs(w[k] - np.linalg.eigvalsh(a[k]))) <= 1e-12 * na
        assert np.linalg.norm(a[k] @ v[k] - v[k] * w[k]) <= 1e-12 * na
        assert np.linalg.norm(v[k].conj().T @ v[k] - np.eye(n)) <= 1e-12
    assert (w[0] < 0).any() and (w[0] > 0).any()  # indefinite


@pytest.mark.gpu
def test_beamformers_more_than_64_microphones_unsupported():
    rng = np.random.default_rng(5)
    csm = np.eye(65, dtype=np.complex128)[None]
    h = rng.standard_normal((1, 65, 10)) + 0j
    for call in (lambda: backend.beamformer_eig_map(csm, h, "mvdr"),
                 lambda: backend.beamformer_cleansc_map(csm, h, 10, 0.5, False),
                 lambda: backend.hermitian_eigh(csm)):
        with pytest.raises(NotImplementedError, match="more than 64 microphones"):
            call()
