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
microphones: a larger array raises NotImplementedError."""

from __future__ import annotations

import numpy as np
from scipy.integrate import simpson

from .. import backend

__all__ = ["delay_and_sum_map", "quadratic_form_map", "BeamformerDASFrequency", "BeamformerCleanSC",
           "BeamformerOrthogonal", "BeamformerFunctional", "BeamformerMVDR"]


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
