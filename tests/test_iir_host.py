"""IIR filters on the host side (no GPU): constructors, conversions and asserts of Filter's IIR forms, the stability
rule, the design helpers against the reference's own output (tests/golden/iir/cases.npz, tools/gen_golden_iir.py),
and a numpy restatement of the device's time-parallel recursion (csrc/kernels_iir.hpp) against scipy."""

import os

import numpy as np
import pytest
import scipy.signal as sig

import dsptoolbox_amd as dsp

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "iir", "cases.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_constructors_and_conversions():
    fs = 48000
    f = dsp.Filter.iir_filter(5, [200.0, 2000.0], dsp.FilterPassType.Bandpass, fs)
    z, p, k = sig.iirfilter(5, [200.0, 2000.0], btype="bandpass", fs=fs, output="zpk")
    assert f.has_zpk and f.has_sos and f.is_iir and not f.is_fir and f.order == 10 and len(f) == 11
    assert np.allclose(f.sos, sig.zpk2sos(z, p, k))
    assert f.metadata == dict(order=10, sampling_rate_hz=fs, filter_type="iir", has_sos=True, has_zpk=True)
    b, a = f.get_coefficients(dsp.FilterCoefficientsType.Ba)
    assert np.allclose(b, sig.sos2tf(f.sos)[0]) and np.allclose(a, sig.sos2tf(f.sos)[1])
    zz, pp, kk = f.get_coefficients(dsp.FilterCoefficientsType.Zpk)
    assert np.array_equal(pp, p) and kk == k
    g = dsp.Filter.from_sos(f.sos, fs)
    assert g.has_sos and not g.has_zpk and g.order == 10
    assert np.allclose(np.sort_complex(g.get_coefficients(dsp.FilterCoefficientsType.Zpk)[1]), np.sort_complex(p))
    h = dsp.Filter.from_zpk(z, p, k, fs)
    assert np.array_equal(h.sos, f.sos)
    # a section with b2 = a2 = 0 counts once
    assert dsp.Filter.from_sos(np.array([[1.0, 0.5, 0.0, 1.0, -0.5, 0.0], [1.0, 0.0, 0.0, 1.0, 0.0, 0.25]]), fs).order == 3
    # ba: sos on demand; an FIR filter stays FIR
    bq = dsp.Filter.biquad(dsp.BiquadEqType.Lowpass, 1000.0, 0.0, 0.7, fs)
    assert bq.is_iir and not bq.has_sos and bq.order == 2
    assert np.allclose(bq.get_coefficients(dsp.FilterCoefficientsType.Sos), sig.tf2sos(*bq.ba))
    with pytest.raises(ValueError):
        bq.get_coefficients("sos")
    with pytest.raises(AssertionError):
        dsp.Filter({dsp.FilterCoefficientsType.Sos: f.sos, dsp.FilterCoefficientsType.Ba: [[1.0], [1.0]]}, fs)
    with pytest.raises(AssertionError):
        dsp.Filter.from_sos(f.sos[0], fs)  # sections must be (n, 6)
    with pytest.raises(AssertionError):
        dsp.Filter.from_sos(f.sos, 48000.0)
    for m in dsp.IirDesignMethod:
        q = dsp.Filter.iir_filter(4, 1000.0, dsp.FilterPassType.Highpass, fs, m, passband_ripple_db=1.0,
                                  stopband_attenuation_db=40.0)
        assert q.has_sos and q.sos.shape == (2, 6)


def test_initial_state_forms():
    fs = 48000
    f = dsp.Filter.iir_filter(4, 1000.0, dsp.FilterPassType.Lowpass, fs).initialize_zi(3)
    assert len(f.zi) == 3 and np.allclose(f.zi[2], sig.sosfilt_zi(f.sos))
    bq = dsp.Filter.biquad(dsp.BiquadEqType.Highpass, 500.0, 0.0, 0.7, fs).initialize_zi(2)
    assert np.allclose(bq.zi[1], sig.lfilter_zi(*bq.ba))


def test_stability_rule():
    fs = 48000
    with pytest.raises(NotImplementedError, match="pole"):
        dsp.Filter({dsp.FilterCoefficientsType.Sos: np.ones((1, 6))}, fs)  # poles on the unit circle
    with pytest.raises(NotImplementedError, match="pole"):
        dsp.Filter.from_ba([1.0], [1.0, -1.5], fs)  # pole at 1.5
    with pytest.raises(NotImplementedError, match="pole"):
        dsp.Filter.from_zpk([], [0.5, 1.0001], 1.0, fs)
    # stable, up to a pole radius of 0.9999
    dsp.Filter.from_zpk([], [0.9999 * np.exp(0.1j), 0.9999 * np.exp(-0.1j)], 1.0, fs)
    dsp.Filter.from_ba([1.0], [1.0, -0.5], fs)
    # FIR filters are not touched by the rule
    assert dsp.Filter.from_ba([1.0, 2.0, 3.0], [1.0], fs).is_fir


def test_unsupported_iir_forms_name_the_limit():
    fs = 48000
    s = dsp.Signal(None, np.zeros((64, 1)), fs)
    high_ba = dsp.Filter.from_ba(*sig.butter(4, 1000.0, fs=fs), fs)
    with pytest.raises(NotImplementedError, match="order > 2"):
        high_ba.filter_signal(s)
    cplx = dsp.Filter.from_ba([1.0 + 1.0j], [1.0, -0.5], fs)
    with pytest.raises(NotImplementedError, match="complex"):
        cplx.filter_signal(s)


def test_fractional_octave_designs_match_reference(golden):
    for b in (1, 3):
        for fs in (44100, 48000):
            bank, c, (lo, hi) = dsp.filterbanks.fractional_octave_bands([31.5, 16e3], b, 6, fs)
            ref_sos, n_sec = golden[f"oct_{b}_{fs}_sos"], golden[f"oct_{b}_{fs}_nsec"]
            assert len(bank) == len(n_sec)
            for i, f in enumerate(bank.filters):
                assert f.sos.shape[0] == n_sec[i]
                np.testing.assert_allclose(f.sos, ref_sos[i, :n_sec[i]], rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(c, golden[f"oct_{b}_{fs}_center"], rtol=1e-14)
            np.testing.assert_allclose(lo, golden[f"oct_{b}_{fs}_lower"], rtol=1e-14)
            np.testing.assert_allclose(hi, golden[f"oct_{b}_{fs}_upper"], rtol=1e-14)
    with pytest.raises(AssertionError):
        dsp.filterbanks.fractional_octave_bands([31.5, 16e3], 1, 6, None)
    with pytest.raises(AssertionError):
        dsp.filterbanks.fractional_octave_bands([31.5, 30e3], 1, 6, 48000)
    # other fractions: exact frequencies only
    nom, ex = dsp.tools.fractional_octave_frequencies(2, (100.0, 1000.0))
    assert nom.size == 0 and np.allclose(ex, 1000.0 * 2 ** (np.arange(-7, 1) / 2))
    with pytest.raises(ValueError):
        dsp.tools.fractional_octave_frequencies(1, (1000.0, 100.0))


def test_biquads_match_reference(golden):
    for t in dsp.BiquadEqType:
        f = dsp.Filter.biquad(t, 1000.0, 4.5, 0.9, 48000)
        b, a = f.get_coefficients(dsp.FilterCoefficientsType.Ba)
        got = np.stack([np.pad(b, (0, 3 - len(b))), np.pad(a, (0, 3 - len(a)))])
        np.testing.assert_allclose(got, golden[f"biquad_{t.name}"], rtol=1e-13, atol=1e-15, err_msg=t.name)


# ---- the device algorithm restated in numpy ----------------------------------------------------------------------
L, B = 32, 64  # samples per block, blocks per group (carry_tables.hpp)


def _cascade(sos, x, state):
    """Serial TDF-II cascade over x from `state` (D,), returns (y, final state)."""
    y = np.array(x, dtype=np.float64)
    st = state.copy()
    for k, (b0, b1, b2, a0, a1, a2) in enumerate(sos):
        b0, b1, b2, a1, a2 = b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0
        z1, z2 = st[2 * k], st[2 * k + 1]
        for i in range(len(y)):
            xi = y[i]
            yi = b0 * xi + z1
            z1 = b1 * xi - a1 * yi + z2
            z2 = b2 * xi - a2 * yi
            y[i] = yi
        st[2 * k], st[2 * k + 1] = z1, z2
    return y, st


def _transition(sos):
    """A: one zero-input step of the cascade's state (column j from the unit state e_j)."""
    d = 2 * len(sos)
    return np.stack([_cascade(sos, [0.0], np.eye(d)[j])[1] for j in range(d)], axis=1)


def _block_parallel(sos, x, zi):
    """Pass 1: every block's final state from zero; pass 2: the carry S_{b+1} = Phi S_b + s_b over groups of B
    blocks (Phi^B between groups) from zi; pass 3: every block rerun from its entry state."""
    d = 2 * len(sos)
    n = len(x)
    nb = -(-n // L)
    blocks = [x[b * L:(b + 1) * L] for b in range(nb)]
    s = np.stack([_cascade(sos, blk, np.zeros(d))[1] for blk in blocks])
    phi = np.linalg.matrix_power(_transition(sos), L)
    phig = np.linalg.matrix_power(phi, B)
    n_groups = -(-nb // B)
    t = []  # zero-entry state of each group
    for g in range(n_groups):
        acc = np.zeros(d)
        for b in range(g * B, min(nb, (g + 1) * B)):
            acc = phi @ acc + s[b]
        t.append(acc)
    entry = np.empty((nb, d))
    tg = zi.copy()
    for g in range(n_groups):
        sg = tg.copy()
        for b in range(g * B, min(nb, (g + 1) * B)):
            entry[b] = sg
            sg = phi @ sg + s[b]
        tg = phig @ tg + t[g]
    outs, zf = [], None
    for b in range(nb):
        yb, zf = _cascade(sos, blocks[b], entry[b])
        outs.append(yb)
    return np.concatenate(outs), zf


# The carry rounds the states once per block and per group; the serial recursion in the same order matches sosfilt
# exactly.  Measured deviation relative to the output's peak: 1.3e-12 (radius 0.999), 2.8e-11 (0.9999) -- DESIGN
# section 9.  The lengths around a multiple of the block and of the group (where the last block is full, the last
# group holds one sample, or there is one group only) are held at radius 0.99 to the bound of radius 0.999: two orders
# inside the 1e-9 the device is held to at the same lengths (test_iir_gpu.py).
EDGE_LENGTHS = [L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, L * B - 1, L * B, L * B + 1, 2 * L * B - 1, 2 * L * B,
                2 * L * B + 1]


@pytest.mark.parametrize("n_sec,n,radius,tol", [(1, 1000, 0.9, 1e-12), (3, 5 * L * B + 17, 0.999, 1e-11),
                                                (4, 2 * L * B + 3 * L, 0.9999, 1e-10)] +
                         [(3, n, 0.99, 1e-11) for n in EDGE_LENGTHS])
def test_block_carry_algebra_matches_sosfilt(n_sec, n, radius, tol):
    rng = np.random.default_rng(n_sec)
    poles = radius * np.exp(1j * rng.uniform(0.001, 0.5, n_sec))
    zeros = np.exp(1j * rng.uniform(0, np.pi, n_sec))
    sos = sig.zpk2sos(np.concatenate([zeros, zeros.conj()]), np.concatenate([poles, poles.conj()]), 1e-3)
    x = rng.standard_normal(n)
    zi = rng.standard_normal((n_sec, 2))
    ref, ref_zf = sig.sosfilt(sos, x, zi=zi)
    got, zf = _block_parallel(sos, x, zi.reshape(-1))
    assert np.max(np.abs(got - ref)) <= tol * np.max(np.abs(ref))
    assert np.max(np.abs(zf - ref_zf.reshape(-1))) <= tol * np.max(np.abs(ref_zf))


def test_carry_tables_under_sanitizers(tmp_path):
    """tests/host_san/carry_tables_san.cpp: csrc/carry_tables.hpp -- A of a cascade, Phi = A^32 and Phi^64 by squaring --
    under AddressSanitizer and UBSan, for real cascades of 1, 3 and 32 sections, complex cascades of 1 and 16 sections and
    a plain matrix with D = 63, against the same powers formed in long double by 31, then 2047, plain multiplications;
    the bound, four times the largest error measured, is in the program's header.  A table squared one time too few and
    the powers of the transposed A must miss it."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "carry_tables_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(root, "tests", "host_san", "carry_tables_san.cpp")], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "carry_tables_san: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    for case in ("real, 1 sections", "real, 3 sections", "real, 32 sections", "complex, 1 sections",
                 "complex, 16 sections", "plain matrix, D = 63"):
        assert case in r.stdout
