"""beamforming: the delay-and-sum map on the cross-spectral matrix
(dsptoolbox/beamforming/beamforming.py:799-880).

The reference's grid / microphone-array / steering-vector classes stay the reference's; what is
replaced is the hot double loop over grid points and frequency bins (:853-858).  A reference
maintainer calls `delay_and_sum_map(f, csm, h, remove_csm_diagonal)` with the selected bins
`f[id1:id2]`, the CSM slice `csm[id1:id2]` (before the diagonal treatment) and the steering
vectors `h = st_vec.get_vector(...)` and gets the integrated map vector back.

BeamformerCleanSC, BeamformerOrthogonal, BeamformerFunctional and BeamformerMVDR (:883-1314) take the
reference's host CSM (`Signal.get_csm()`: cached, float64 for short estimates), upload only the selected
bins with their steering vectors and run the whole per-bin method on the device in float64 (one Hermitian
eigendecomposition per bin for MVDR / Functional / Orthogonal, the CLEAN-SC loop for CleanSC).  Up to 64
microphones: a larger array raises NotImplementedError.

BeamformerDASTime (:1317-1394), MonopoleSource (:1397-1464) and mix_sources_on_array (:1467-1512) are sums of
fractionally delayed channels: one ds_delay_sum launch builds every (grid point, microphone) filter and adds the
delayed channels up, where the reference runs one fractional_delay per pair in a Python double loop."""

from __future__ import annotations

from warnings import warn

import numpy as np
from scipy.integrate import simpson

from .. import backend

__all__ = ["delay_and_sum_map", "quadratic_form_map", "BeamformerDASFrequency", "BeamformerCleanSC",
           "BeamformerOrthogonal", "BeamformerFunctional", "BeamformerMVDR", "BeamformerDASTime", "MonopoleSource",
           "mix_sources_on_array"]


def quadratic_form_map(csm, h) -> np.ndarray:
    """map[g, f] = Re(h[f, :, g]^H csm[f] h[f, :, g]) on the device (fp32 MFMA).
    csm (F, C, C), h (F, C, G) complex -> (G, F) float64."""
    return backend._das_map(csm, h)


def delay_and_sum_map(f, csm, h, remove_csm_diagonal: bool = True) -> np.ndarray:
    """Frequency-domain delay-and-sum map integrated over the bins `f` (:838-876)."""
    f = np.asarray(f, dtype=np.float64)
    csm = np.array(csm, dtype=np.complex128)  # the reference scales / zeroes its CSM in place: copy
    n_ch = csm.shape[1]
    if remove_csm_diagonal:
        csm *= n_ch / (n_ch - 1)  # account for energy loss
        for i in range(len(f)):
            np.fill_diagonal(csm[i, :, :], 0)
    m = quadratic_form_map(csm, h)
    if remove_csm_diagonal:
        m[m < 0] = 0  # unphysical values for the removed diagonal
    if len(f) > 1:
        return simpson(m, dx=f[1] - f[0], axis=1)
    return m.squeeze()


class _GriddedBeamformer:
    """What the gridded frequency-domain beamformers share (beamforming.py:760-796): the constructor, the CSM
    parameters, the band selection and the integration over the selected bins."""

    def __init__(self, multi_channel_signal, mic_array, grid, steering_vector, c: float = 343):
        assert multi_channel_signal.number_of_channels > 1, "Signal must be multichannel"
        assert c > 0, "Speed of sound should be bigger than 0"
        assert hasattr(steering_vector, "get_vector"), "steering_vector should offer get_vector()"
        assert hasattr(grid, "number_of_points") and hasattr(grid, "reconstruct_map_shape"), "grid should be a Grid object"
        self.signal, self.mics, self.grid, self.st_vec, self.c = multi_channel_signal, mic_array, grid, steering_vector, c

    def set_csm_parameters(self, **kwargs):
        """Spectrum parameters of the multi-channel signal's CSM (Signal.set_spectrum_parameters)."""
        self.signal.set_spectrum_parameters(**kwargs)

    def _set_band(self, center_frequency_hz: float, octave_fraction: int):
        self.center_frequency_hz, self.octave_fraction = center_frequency_hz, octave_fraction
        # helpers/other.py:156-178
        self.f_range_hz = (np.array([center_frequency_hz, center_frequency_hz]) if octave_fraction == 0 else
                           np.array([center_frequency_hz * 2 ** (-1 / octave_fraction / 2),
                                     center_frequency_hz * 2 ** (1 / octave_fraction / 2)]))

    def _select_bins(self, f):
        """-> (id1, id2, f[id1:id2], steering vectors of those bins); f_range_hz becomes the bins' range."""
        from ..transfer_functions import find_nearest_points_index_in_vector
        ids = find_nearest_points_index_in_vector(self.f_range_hz, f)
        id1, id2 = int(ids[0]), int(ids[1])
        if id1 == id2:
            id2 += 1
        f = f[id1:id2]
        wave_numbers = f * np.pi * 2 / self.c
        h = self.st_vec.get_vector(wave_numbers, grid=self.grid, mic=self.mics)
        self.f_range_hz = np.array([f[0], f[-1]])
        return id1, id2, f, h

    def _finish(self, m, f) -> np.ndarray:
        m = simpson(m, dx=f[1] - f[0], axis=1) if len(f) > 1 else m.squeeze()
        self.map = self.grid.reconstruct_map_shape(m)
        return self.map.copy()

    def _host_band(self, center_frequency_hz: float, octave_fraction: int):
        """The reference's CSM (Signal.get_csm) and steering vectors for the selected bins."""
        self._set_band(center_frequency_hz, octave_fraction)
        f, csm = self.signal.get_csm()
        id1, id2, f, h = self._select_bins(f)
        return f, csm[id1:id2], h


class BeamformerDASFrequency(_GriddedBeamformer):
    """Frequency-domain delay-and-sum beamformer with the reference's interface
    (beamforming/beamforming.py:760-880): built from a multi-channel Signal, a microphone array, a grid and
    a steering vector -- the reference's own geometry objects, or anything that offers
    `steering_vector.get_vector(wave_numbers, grid=, mic=) -> (bins, channels, grid points)`,
    `grid.number_of_points` and `grid.reconstruct_map_shape(map)`.  The cross-spectral matrix is computed
    on the device and STAYS there (Signal.get_csm(on_device=True)); the diagonal treatment and the
    grid x bin quadratic forms run on it in place; only the steering vectors travel up and the map down."""

    beamformer_type = "Delay-and-sum (Frequency)"

    def get_beamformer_map(self, center_frequency_hz: float, octave_fraction: int = 3,
                           remove_csm_diagonal: bool = True) -> np.ndarray:
        self._set_band(center_frequency_hz, octave_fraction)
        f, csm = self.signal.get_csm(on_device=True)
        try:
            id1, id2, f, h = self._select_bins(f)
            m = backend._das_map_device(csm, id1, id2, h, remove_csm_diagonal)
        finally:
            csm.free()
        if remove_csm_diagonal:
            m[m < 0] = 0  # unphysical values for the removed diagonal
        return self._finish(m, f)


class BeamformerCleanSC(_GriddedBeamformer):
    """CLEAN-SC (Sijtsma 2007) with the reference's interface (beamforming.py:883-1007): the dirty map
    Re(h^H D h), then per bin at most `maximum_iterations` rounds of peak pick, source-coherent point
    spread removal and CSM degradation, all on the device (ds_bf_cleansc).  Returns the clean map."""

    beamformer_type = "CleanSC"

    def get_beamformer_map(self, center_frequency_hz: float, octave_fraction: int = 3,
                           maximum_iterations: int | None = None, safety_factor: float = 0.5,
                           remove_csm_diagonal: bool = False) -> np.ndarray:
        if maximum_iterations is None:
            maximum_iterations = self.signal.number_of_channels * 2
        else:
            assert maximum_iterations > 0, "Number of iterations must be positive"
        assert safety_factor > 0 and safety_factor <= 1, (
            f"{safety_factor} is not valid. The safety factor (loop gain) should be in ]0, 1]")
        f, csm, h = self._host_band(center_frequency_hz, octave_fraction)
        m = backend.beamformer_cleansc_map(csm, h, maximum_iterations, safety_factor, remove_csm_diagonal)
        return self._finish(m, f)


class BeamformerOrthogonal(_GriddedBeamformer):
    """Orthogonal beamforming (Sarradj 2010) with the reference's interface (beamforming.py:1010-1124): per bin
    and for each of the `number_eigenvalues` largest (signed) eigenvalues, the grid point where the eigenvector's
    map |h^H v|^2 peaks gets that value times the eigenvalue (ds_bf_eig_map, method 2)."""

    beamformer_type = "Orthogonal (Grid)"

    def get_beamformer_map(self, center_frequency_hz: float, octave_fraction: int = 3,
                           number_eigenvalues: int | None = None) -> np.ndarray:
        if number_eigenvalues is None:
            number_eigenvalues = self.signal.number_of_channels // 2
        else:
            assert number_eigenvalues <= self.signal.number_of_channels, (
                "Number of eigenvalues cannot be more than number of microphones")
            assert number_eigenvalues > 0, "At least one eigenvalue of the CSM must be regarded"
        f, csm, h = self._host_band(center_frequency_hz, octave_fraction)
        m = backend.beamformer_eig_map(csm, h, "orthogonal", n_eig=number_eigenvalues)
        return self._finish(m, f)


class BeamformerFunctional(_GriddedBeamformer):
    """Functional beamforming (Dougherty 2014) with the reference's interface (beamforming.py:1127-1220):
    map = (h^H CSM^(1/gamma) h / h^H h)^gamma h^H h, the matrix power taken through the SVD as the reference
    does -- sign(lambda)|lambda|^(1/gamma) on an indefinite CSM (ds_bf_eig_map, method 1)."""

    beamformer_type = "Functional"

    def get_beamformer_map(self, center_frequency_hz: float, octave_fraction: int = 3,
                           gamma: float = 10) -> np.ndarray:
        f, csm, h = self._host_band(center_frequency_hz, octave_fraction)
        m = backend.beamformer_eig_map(csm, h, "functional", gamma=gamma)
        return self._finish(m, f)


class BeamformerMVDR(_GriddedBeamformer):
    """MVDR (Capon) beamforming with the reference's interface (beamforming.py:1223-1314):
    map = 1 / Re(h^H CSM^-1 h), the inverse applied through the eigendecomposition (ds_bf_eig_map, method 0).
    `gamma` is accepted and ignored, as in the reference."""

    beamformer_type = "MVDR"

    def get_beamformer_map(self, center_frequency_hz: float, octave_fraction: int = 3,
                           gamma: float = 10) -> np.ndarray:
        f, csm, h = self._host_band(center_frequency_hz, octave_fraction)
        m = backend.beamformer_eig_map(csm, h, "mvdr")
        return self._finish(m, f)


# ---- time domain: sums of fractionally delayed channels (ds_delay_sum) ---------------------------------------------
_DELAY_ORDER = 30  # fractional_delay's defaults, which the reference's time-domain code uses
_DELAY_SIDE_LOBES_DB = 60


class BeamformerDASTime:
    """Delay-and-sum beamformer in the time domain with the reference's interface (beamforming.py:1317-1394): every
    microphone is delayed to the farthest one for each grid point, scaled by its distance and averaged.  `mic_array`
    offers `get_distances_to_point(points) -> (mics, points)` and `number_of_points`, `grid` offers
    `number_of_points` and `coordinates`.  The whole grid is one device launch (ds_delay_sum): G * M Kaiser-sinc
    filters of order 30 and the weighted sum, float64.  A device-resident signal that does not constrain its
    amplitude gives a device-resident output."""

    beamformer_type = "Delay-and-sum (Time)"

    def __init__(self, multi_channel_signal, mic_array, grid, c: float = 343):
        from ..classes import Signal
        assert isinstance(multi_channel_signal, Signal), "Multi-channel signal must be of type Signal"
        assert hasattr(mic_array, "get_distances_to_point"), "mic_array should be of type MicArray"
        assert c > 0, "Speed of sound should be bigger than 0"
        assert multi_channel_signal.number_of_channels == mic_array.number_of_points, \
            "Number of channels in signal and microphone array do not match"
        assert hasattr(grid, "number_of_points") and hasattr(grid, "coordinates"), "grid should be a Grid object"
        self.signal, self.mics, self.grid, self.c = multi_channel_signal, mic_array, grid, c

    def _terms(self):
        """-> (rows G x terms M: shift, frac, weight before the 1 / M, distances (M, G), output length)."""
        from .. import backend
        n_mics, n_grid = self.mics.number_of_points, self.grid.number_of_points
        ds = np.asarray(self.mics.get_distances_to_point(self.grid.coordinates), dtype=np.float64)
        ds = ds.reshape(n_mics, n_grid)
        min_distance, r0 = np.min(ds), np.max(ds)
        fs = self.signal.sampling_rate_hz
        longest = int((r0 - min_distance) / self.c * fs + 2)
        total = self.signal.length_samples + longest
        delays = (r0 - ds.T) / self.c  # (G, M), the reference's delays[im] for grid point ig
        integer_delay, frac = backend._delay_split(delays * fs, _DELAY_ORDER)
        zero = delays == 0  # fractional_delay's sig.copy(): unshifted, no filter
        shift = np.where(zero, 0, integer_delay)
        frac = np.where(zero, -1.0, frac)
        return shift, frac, ds, total

    def get_beamformer_output(self):
        """-> Signal with one channel per grid point, focused there (total length: the input's plus the longest
        delay plus 2 samples)."""
        from .. import backend
        sig = self.signal
        shift, frac, ds, total = self._terms()
        n_mics, n_grid = ds.shape
        n = sig.length_samples
        src = np.broadcast_to(np.arange(n_mics, dtype=np.int32), (n_grid, n_mics))
        if sig.on_device and not sig.constrain_amplitude:
            dev = backend.delay_sum_device(sig.device_samples, n, src, shift, frac, ds.T / n_mics, _DELAY_ORDER,
                                           _DELAY_SIDE_LOBES_DB, total)
            return sig._device_result(dev)
        weight = ds.T / n_mics
        if sig.constrain_amplitude:
            # each delayed microphone signal is a Signal of its own in the reference: one above 0 dBFS is normalised
            # to its peak before it is weighted (full length: N + order + integer_delay, or N for a pass-through)
            _, p_pair = backend.delay_sum(sig.time_data, n, src.reshape(-1, 1), shift.reshape(-1, 1),
                                          frac.reshape(-1, 1), 1.0, _DELAY_ORDER, _DELAY_SIDE_LOBES_DB,
                                          n + _DELAY_ORDER + max(int(shift.max()), 0), want_samples=False,
                                          want_peaks=True)
            weight = ds.T / np.maximum(1.0, p_pair.reshape(n_grid, n_mics)) / n_mics
        y, peaks = backend.delay_sum(sig.time_data, n, src, shift, frac, weight, _DELAY_ORDER, _DELAY_SIDE_LOBES_DB,
                                     total, want_peaks=sig.constrain_amplitude)
        if sig.constrain_amplitude:
            # The reference adds the grid points one add_channel at a time; each addition whose channel peaks above 1
            # divides every channel so far by that peak.  Channel g thus ends up divided by prod_{i >= g} max(1, p_i).
            scale = np.maximum(1.0, peaks)
            if np.any(scale > 1.0):
                warn("Signal was over 0 dBFS, normalizing to 0 dBFS peak level was triggered")
            y /= np.cumprod(scale[::-1])[::-1][None, :]
        return sig.copy_with_new_time_data(y)  # (peaks at most 1 now: a constrained copy leaves it as it is)


class MonopoleSource:
    """A source with an omnidirectional emission (beamforming.py:1397-1464): a one-channel Signal at `coordinates`
    (x, y, z)."""

    def __init__(self, signal, coordinates):
        assert signal.number_of_channels == 1, "Only signals with a single channel are supported"
        coordinates = np.squeeze(coordinates)
        assert len(coordinates) == 3 and coordinates.ndim == 1, "Coordinates should have exactly three values"
        self.emitted_signal = signal
        self.coordinates = coordinates

    def _terms(self, mics, c: float):
        from .. import backend
        distances = np.atleast_1d(np.asarray(mics.get_distances_to_point(self.coordinates), dtype=np.float64))
        delays = distances / c
        fs = self.emitted_signal.sampling_rate_hz
        n = self.emitted_signal.length_samples
        assert np.all(delays >= 0), "Delay must be positive"
        assert np.all(delays * fs < n), "Delay too large for the given signal"
        integer_delay, frac = backend._delay_split(delays * fs, _DELAY_ORDER)
        zero = delays == 0
        return distances, np.where(zero, 0, integer_delay), np.where(zero, -1.0, frac)

    def get_signals_on_array(self, mics, c: float = 343):
        """The emitted signal at every microphone: delayed by distance / c (keeping its length) and scaled by
        1 / (1 + distance).  One device launch for all microphones."""
        from .. import backend
        sig = self.emitted_signal
        distances, shift, frac = self._terms(mics, c)
        n = sig.length_samples
        src = np.zeros((len(distances), 1), dtype=np.int32)
        if sig.on_device and not sig.constrain_amplitude:
            dev = backend.delay_sum_device(sig.device_samples, n, src, shift[:, None], frac[:, None],
                                           (1.0 / (1.0 + distances))[:, None], _DELAY_ORDER, _DELAY_SIDE_LOBES_DB, n)
            return sig._device_result(dev)
        y, _ = backend.delay_sum(sig.time_data, n, src, shift[:, None], frac[:, None], 1.0, _DELAY_ORDER,
                                 _DELAY_SIDE_LOBES_DB, n)
        if sig.constrain_amplitude:  # every delayed copy is a constrained Signal of its own in the reference
            peaks = np.max(np.abs(y), axis=0)
            over = (peaks > 1.0) & (frac >= 0)
            if np.any(over):
                warn("Signal was over 0 dBFS, normalizing to 0 dBFS peak level was triggered")
                y[:, over] /= peaks[over]
        y /= (1.0 + distances)[None, :]
        return sig.copy_with_new_time_data(y)  # (normalises a constrained result above 0 dBFS)


def mix_sources_on_array(sources, mics, c: float = 343):
    """The multi-channel signal of several MonopoleSource on the array (beamforming.py:1467-1512): the first source
    is delayed from its whole signal, every later one after trimming it (and the mix so far) to the shortest length
    seen -- with the reference's warning, and with its pop(0) on the caller's list and the trimmed emitted signals
    left in the sources.  Device-resident, unconstrained sources are mixed in one launch (one term per source)."""
    from .. import backend
    if type(sources) is MonopoleSource:
        sources = [sources]
    assert len(sources) > 0, "There must be at least one source to project on array"
    assert all([type(i) is MonopoleSource for i in sources]), "All sources in list should be of type Source"
    first = sources[0]
    resident = all(s.emitted_signal.on_device and not s.emitted_signal.constrain_amplitude for s in sources)
    total = first.emitted_signal.length_samples
    lengths = [total]
    for s in sources[1:]:
        if total != s.emitted_signal.length_samples:
            warn("Emitted signals from sources differ in length. Trimming to shortest will be done")
            total = min(total, s.emitted_signal.length_samples)
            if s.emitted_signal.length_samples != total:
                s.emitted_signal = _pad_trim_signal(s.emitted_signal, total)
        lengths.append(total)
    sources.pop(0)
    everyone = [first] + list(sources)
    if not resident:
        mixed = first.get_signals_on_array(mics, c)
        for s, n_s in zip(sources, lengths[1:]):
            if mixed.length_samples != n_s:
                mixed = _pad_trim_signal(mixed, n_s)
            mixed.time_data = mixed.time_data + s.get_signals_on_array(mics, c).time_data
        return mixed
    # one launch: microphone g sums term j = source j, read over its own length
    terms = [s._terms(mics, c) for s in everyone]
    n_mics = len(terms[0][0])
    stacked = backend.stack_device([s.emitted_signal.device_samples for s in everyone], lengths)
    src = np.broadcast_to(np.arange(len(everyone), dtype=np.int32), (n_mics, len(everyone)))
    shift = np.stack([t[1] for t in terms], axis=1)
    frac = np.stack([t[2] for t in terms], axis=1)
    weight = np.stack([1.0 / (1.0 + t[0]) for t in terms], axis=1)
    dev = backend.delay_sum_device(stacked, np.asarray(lengths), src, shift, frac, weight, _DELAY_ORDER,
                                   _DELAY_SIDE_LOBES_DB, total)
    return first.emitted_signal._device_result(dev)


def _pad_trim_signal(signal, length: int):
    """standard.pad_trim at the end (pad_trim_methods.py:12-48) for a Signal; a device-resident, unconstrained signal
    is trimmed as a view of its samples."""
    from .. import backend
    from .._lib import DevicePlanar
    if signal.on_device and not signal.constrain_amplitude and length <= signal.length_samples:
        d = signal.device_samples
        return signal._device_result(DevicePlanar(d.owner, d.n_ch, length, d.ld, d.offset_bytes))
    return signal.copy_with_new_time_data(backend._pad_trim(signal.time_data, length))
