"""Fractional delays without a GPU: the exports, the reference's asserts, and the host-side split of a delay into
the integer shift and fraction (with the output lengths that follow) against a numpy restatement of the reference's
_fractional_delay_filter (standard/_standard_backend.py:430-492) and fractional_delay (latency_delay.py:159-285)."""

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd.beamforming import BeamformerDASTime, MonopoleSource, mix_sources_on_array


def ref_split(delay_samples, order):
    """(integer_delay, fraction) exactly as the reference computes them, one delay at a time."""
    delay_int = int(delay_samples)
    delay_frac = delay_samples - delay_int
    if order % 2:
        m_opt = int(delay_frac) - (order - 1) / 2
    else:
        m_opt = np.round(delay_frac) - order / 2
    return int(delay_int + m_opt), delay_frac


def ref_length(n, delay_samples, order, keep_length):
    integer_delay, _ = ref_split(delay_samples, order)
    return n if keep_length else n + order + integer_delay


def test_exports():
    assert dsp.fractional_delay is dsp.standard.fractional_delay
    assert "fractional_delay" in dsp.__all__ and "standard" in dsp.__all__
    assert "fractional_delay" in dsp.standard.__all__
    for name in ("BeamformerDASTime", "MonopoleSource", "mix_sources_on_array"):
        assert name in dsp.beamforming.__all__ and hasattr(dsp.beamforming, name)


@pytest.mark.parametrize("order", [30, 31, 8, 1, 2, 255])
def test_split_matches_reference(order):
    rng = np.random.default_rng(order)
    fs = 48000
    delays = np.concatenate([rng.uniform(0, 0.01, 2000), np.arange(1, 50) / fs, (np.arange(1, 50) + 0.5) / fs,
                             (np.arange(1, 50) - 1e-12) / fs, [0.0001875, 1e-9, 0.3 / fs]])
    d = delays * fs
    shift, frac = backend._delay_split(d, order)
    for k in range(len(d)):
        want_shift, want_frac = ref_split(float(d[k]), order)
        assert shift[k] == want_shift and frac[k] == want_frac, (d[k], order)
        s1, f1 = backend._delay_split(float(d[k]), order)
        assert (s1, f1) == (want_shift, want_frac)


def test_half_sample_rounds_to_even():
    # np.round(0.5) is 0: a fraction of exactly 0.5 does not shift the even-order filter; anything above does
    assert backend._delay_split(10.5, 30)[0] == 10 - 15
    assert backend._delay_split(10.75, 30)[0] == 10 + 1 - 15
    assert backend._delay_split(10.5, 31)[0] == 10 - 15


def test_kaiser_beta():
    assert backend._kaiser_window_beta(60) == pytest.approx(0.1102 * (60 - 8.7))
    assert backend._kaiser_window_beta(-30) == pytest.approx(0.5842 * 9 ** 0.4 + 0.07886 * 9)
    assert backend._kaiser_window_beta(10) == 0.0


@pytest.mark.parametrize("keep", [False, True])
def test_output_lengths(keep):
    from dsptoolbox_amd.standard.latency_delay import _delay_rows
    n, fs = 500, 48000
    for d_s in (10.25 / fs, 10.5 / fs, 0.3 / fs, 3.9 / fs):
        for order in (30, 31, 8):
            shift, frac, integer_delay = _delay_rows(3, np.array([0, 2]), d_s * fs, order)
            assert integer_delay == ref_split(d_s * fs, order)[0]
            assert list(shift) == [integer_delay, 0, integer_delay] and frac[1] < 0 and frac[0] >= 0
            out_len = n if keep else n + order + integer_delay
            assert out_len == ref_length(n, d_s * fs, order, keep)


def _sig(n=200, ch=2):
    return dsp.Signal(None, np.random.default_rng(1).standard_normal((n, ch)), 48000)


def test_asserts():
    s = _sig()
    with pytest.raises(AssertionError, match="Delay must be positive"):
        dsp.fractional_delay(s, -1e-3)
    with pytest.raises(AssertionError, match="Delay too large"):
        dsp.fractional_delay(s, 300 / 48000, keep_length=True)
    with pytest.raises(AssertionError, match="invalid channel"):
        dsp.fractional_delay(s, 1e-4, channels=[0, 2])
    with pytest.raises(AssertionError, match="invalid channel"):
        dsp.fractional_delay(s, 1e-4, channels=[1, 1])
    with pytest.raises(TypeError):
        dsp.fractional_delay(np.zeros(10), 1e-4)
    assert dsp.fractional_delay(s, 0.0).time_data.shape == s.time_data.shape  # the copy: no device needed
    with pytest.raises(AssertionError, match="single channel"):
        MonopoleSource(_sig(ch=2), [0, 0, 1])
    with pytest.raises(AssertionError, match="three values"):
        MonopoleSource(_sig(ch=1), [0, 1])
    with pytest.raises(AssertionError, match="three values"):
        MonopoleSource(_sig(ch=1), np.zeros((2, 3)))
    with pytest.raises(AssertionError, match="at least one source"):
        mix_sources_on_array([], None)
    with pytest.raises(AssertionError, match="type Source"):
        mix_sources_on_array([object()], None)


def test_das_time_asserts():
    class Mics:
        number_of_points = 2

        def get_distances_to_point(self, p):
            return np.ones((2, 1))

    class Grid:
        number_of_points = 1
        coordinates = np.zeros((1, 3))

    with pytest.raises(AssertionError, match="do not match"):
        BeamformerDASTime(_sig(ch=3), Mics(), Grid())
    with pytest.raises(AssertionError, match="Speed of sound"):
        BeamformerDASTime(_sig(ch=2), Mics(), Grid(), c=0)
    with pytest.raises(AssertionError, match="Grid object"):
        BeamformerDASTime(_sig(ch=2), Mics(), object())
