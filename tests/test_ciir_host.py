"""The complex-coefficient recursion and the gammatone bank on the CPU: the clongdouble oracle against the reference's
golden vectors, the bounds of ciir_cases.py measured again from the float64 emulation of the blocked algorithm, the
constants the cases mirror, what the bounds reject, every refusal, and the API surface."""

import os
import re

import numpy as np
import pytest

import ciir_cases as cc
import ciir_oracle as co
import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 8000


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "gammatone", "cases.npz"))


def test_bank_parameters_match_reference():
    z = golden()
    counts = []
    for i in range(4):
        lo, hi, res, fs = z[f"bank{i}_args"]
        fb = dsp.filterbanks.auditory_filters_gammatone([lo, hi], res, int(fs))
        assert type(fb) is dsp.filterbanks.GammaToneFilterBank and isinstance(fb, dsp.FilterBank)
        np.testing.assert_allclose(fb._frequencies, z[f"bank{i}_freq"], rtol=1e-14)
        np.testing.assert_allclose(fb._coefficients, z[f"bank{i}_coef"], rtol=1e-14)
        np.testing.assert_allclose(fb._normalizations, z[f"bank{i}_norm"], rtol=1e-12)
        np.testing.assert_allclose(dsp.tools.erb_frequencies([lo, hi], res), z[f"bank{i}_freq"], rtol=1e-14)
        counts.append(len(fb))
        for f, a, g in zip(fb.filters, fb._coefficients, fb._normalizations):
            want = np.tile(np.array([1, 0, 0, 1, -a, 0]), (4, 1))
            want[3, 0] = g
            assert np.array_equal(f.sos, want) and f.warning_if_complex is False
        assert fb.info == {"Type of filter bank": "Gammatone filter bank"} and fb.same_sampling_rate
    assert counts[:3] == [23, 30, 40]
    assert np.array_equal(dsp.tools.erb_frequencies([3500, 100], 1), z["bank0_freq"])  # (limits in either order)


def test_bank_assertions_and_reconstruct():
    with pytest.raises(AssertionError, match="sampling rate must be passed"):
        dsp.filterbanks.auditory_filters_gammatone([100, 3500])
    with pytest.raises(AssertionError, match="nyquist"):
        dsp.filterbanks.auditory_filters_gammatone([100, 4001], 1, 8000)
    with pytest.raises(ValueError, match="length 2"):
        dsp.tools.erb_frequencies([100, 200, 300])
    with pytest.raises(ValueError, match="larger than zero"):
        dsp.tools.erb_frequencies([100, 3500], 0)
    fb = dsp.filterbanks.auditory_filters_gammatone([900, 1100], 1, FS)
    with pytest.raises(NotImplementedError, match="NaN"):
        fb.reconstruct(None)


def test_oracle_reproduces_the_reference():
    """scipy's complex sosfilt (the golden vectors) against the clongdouble recursion: both within a few eps64 of the
    output's peak."""
    z = golden()
    x = z["x"].astype(np.float64)
    worst = 0.0
    for key, f_range, chans in (("par", [700, 1500], slice(0, 2)), ("zi1", [900, 1100], slice(0, 2))):
        sos = cc.gammatone_sos(f_range, FS)
        zi = None
        if key == "zi1":
            from scipy.signal import sosfilt_zi
            zi = np.stack([np.repeat(sosfilt_zi(s)[:, :, None], 2, axis=2) for s in sos])
        y, zf = co.bank_ld(sos, x[:, chans], zi)
        for k in range(len(sos)):
            worst = max(worst, co.stream_error(z[key][k], y[k]))
        if key == "zi1":
            # the reference keeps the unpacked (sections, 2, channels) state array, whose length is not the channel
            # count: its second call starts from the steady state again (as with real sections, test_iir_host.py)
            for k in range(len(sos)):
                worst = max(worst, co.stream_error(z["zi2"][k], y[k]))
    f0 = cc.gammatone_sos([900, 1100], FS)[0]
    worst = max(worst, co.stream_error(z["single"], co.sosfilt_ld(f0, x[:, :2])[0]))
    sub = co.sosfilt_ld(f0, x[:, 1:2])[0]
    worst = max(worst, co.stream_error(z["sub"][:, 1:2], sub))
    assert np.array_equal(z["sub"][:, [0, 2]], x[:, [0, 2]].astype(np.complex128))  # (the other channels pass through)
    print(f"the reference's outputs against the clongdouble oracle: {worst:.2e} of the peak")
    assert worst <= 16 * cc.EPS


@pytest.mark.parametrize("name", list(cc.RECURSION))
def test_emulation_gives_the_recorded_bound(name):
    e = cc.recursion_error(name, *cc.emulate_recursion(name)) / cc.EPS
    rec = cc.CIIR_EMULATION[name]
    print(f"{name}: emulation {e:.3g} eps64 (recorded {rec:.3g}), bound {cc.recursion_tolerance(name):.2e}")
    assert rec / cc.HOST_MARGIN / 2 <= e <= rec * cc.HOST_MARGIN, (name, e, rec)
    assert cc.recursion_tolerance(name) <= 1e-11  # (nothing looser than the suite's float64 routes)


@pytest.mark.parametrize("name", ["one_pole_near0_n4097", "gammatone23_n4097_zi", "max_sections_n4097_zi"])
def test_bound_rejects_broken_carries(name):
    tol = cc.recursion_tolerance(name)
    off = cc.recursion_error(name, *cc.emulate_recursion(name, phi_power_offset=1))
    flat = cc.recursion_error(name, *cc.emulate_recursion(name, drop_imag_state=True))
    print(f"{name}: Phi one power off {off:.2e}, imaginary state dropped {flat:.2e}, bound {tol:.2e}")
    assert off > 100 * tol and flat > 100 * tol


def _header_constant(header, name):
    src = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", header)).read()
    m = re.search(r"constexpr int %s = ([^;]+);" % name, src)
    assert m, (header, name)
    return eval(m.group(1), {"NT": 256, "PER_LANE": 16})


def test_case_constants_match_the_sources():
    assert _header_constant("carry_tables.hpp", "L") == cc.L and _header_constant("carry_tables.hpp", "B") == cc.B
    assert _header_constant("kernels_ciir.hpp", "CIIR_MAX_SEC") == cc.CIIR_MAX_SEC == backend.CIIR_MAX_SEC
    assert _header_constant("kernels_dist.hpp", "NT") == cc.PAIR_NT
    assert _header_constant("kernels_dist.hpp", "SPAN") == cc.PAIR_SPAN == backend.PAIR_SPAN
    src = open(os.path.join(ROOT, "tests", "test_phase_gpu.py")).read()
    assert float(re.search(r"^TOL = (\S+)", src, re.M).group(1)) == cc.FFT_TOL
    api = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "api.hip")).read()
    assert "more than 16 complex second-order sections" in api and cc.CIIR_MAX_SEC == 16


# ---- the refusals: each names its limit and none reaches the device -------------------------------------------------------
def _signal(n_ch=1, n=64):
    return dsp.Signal(None, np.random.default_rng(0).standard_normal((n, n_ch)), FS, constrain_amplitude=False)


def _band():
    return dsp.filterbanks.auditory_filters_gammatone([900, 1100], 1, FS).filters[0]


def test_refusals_name_their_limits():
    s, band = _signal(), _band()
    real = dsp.Filter.iir_filter(2, 1000.0, dsp.FilterPassType.Lowpass, FS)
    fir = dsp.Filter.fir_filter(8, 1000.0, dsp.FilterPassType.Lowpass, FS)
    with pytest.raises(NotImplementedError, match="complex"):  # complex ba
        dsp.Filter.from_ba([1.0 + 1.0j], [1.0, -0.5], FS).filter_signal(s)
    with pytest.raises(NotImplementedError, match="zero-phase"):
        band.filter_signal(s, zero_phase=True)
    bank = dsp.FilterBank([band, _band()])
    for mode in (dsp.FilterBankMode.Summed, dsp.FilterBankMode.Sequential):
        with pytest.raises(NotImplementedError, match="Summed and Sequential"):
            bank.filter_signal(s, mode)
        with pytest.raises(NotImplementedError, match="Summed and Sequential"):
            bank.filter_signal(s, mode, activate_zi=True)
    with pytest.raises(NotImplementedError, match="zero-phase"):
        bank.filter_signal(s, dsp.FilterBankMode.Parallel, zero_phase=True)
    for other in (real, fir):
        with pytest.raises(NotImplementedError, match="mixing"):
            dsp.FilterBank([band, other]).filter_signal(s, dsp.FilterBankMode.Parallel)
    cs = dsp.Signal(None, np.ones((64, 1)) + 0.5j, FS, constrain_amplitude=False)
    assert cs.is_complex_signal
    with pytest.raises(NotImplementedError, match="complex input"):
        band.filter_signal(cs)
    with pytest.raises(NotImplementedError, match="complex input"):
        bank.filter_signal(cs, dsp.FilterBankMode.Parallel)
    with pytest.raises(NotImplementedError, match="complex input"):
        backend.iir_sos_filter_complex(np.ones((8, 1)) + 1j, [band.sos])
    long = dsp.Filter.from_sos(np.tile(band.sos[:1], (cc.CIIR_MAX_SEC + 1, 1)), FS)
    with pytest.raises(NotImplementedError, match=f"more than {cc.CIIR_MAX_SEC}"):
        long.filter_signal(s)
    with pytest.raises(NotImplementedError, match=f"more than {cc.CIIR_MAX_SEC}"):
        backend.iir_sos_filter_complex(np.ones((8, 1)), [long.sos])
    assert dsp.Filter.from_sos(np.tile(band.sos[:1], (cc.CIIR_MAX_SEC, 1)), FS)._device_sections().dtype == np.complex128


def test_unstable_complex_sections_raise_when_built():
    sos = np.array([[1, 0, 0, 1, -1.0001 * np.exp(0.3j), 0]])
    with pytest.raises(NotImplementedError, match="pole of magnitude"):
        dsp.Filter.from_sos(sos, FS)
    with pytest.raises(NotImplementedError, match="pole of magnitude"):
        dsp.Filter.from_sos(np.array([[1, 0, 0, 1, -1.0 + 0j, 0]]), FS)  # (on the circle)


def test_api_surface():
    assert "distances" in dsp.__all__ and dsp.distances.__all__ == ["log_spectral", "itakura_saito", "snr", "si_sdr",
                                                                    "fw_snr_seg"]
    assert {"auditory_filters_gammatone", "GammaToneFilterBank"} <= set(dsp.filterbanks.__all__)
    assert callable(dsp.tools.erb_frequencies) and callable(backend.iir_sos_filter_complex)
    from dsptoolbox_amd._lib import SIGNATURES
    assert {"ds_iir_sos_c128", "ds_pair_moments", "ds_pair_moments_dev", "ds_fw_snr_seg", "ds_fw_snr_seg_dev"} <= set(SIGNATURES)
    assert backend.FW_SNR_CHUNK_FRAMES >= 1
