"""Room and ShoeboxRoom of the reference (room_acoustics/_room_acoustics.py:272-837) with its constructors, assertions
and messages.  The attributes are host arithmetic; the modal sum of get_analytical_transfer_function runs on the device
(backend.room_modal_response) over a table of modes built here, vectorised, in the reference's loop order."""

from __future__ import annotations

import numpy as np

from .. import backend

_WALLS = {"north": 0, "south": 1, "east": 2, "west": 3, "floor": 4, "ceiling": 5}
_README = """This dictionary contains all information about the room's
absorption properties. Its keys are:

- absorption_matrix : array containing absorption with shape
(wall, frequency band) = (6, number of bands). Frequencies are in increasing
order and walls indices can be retrieved with the
index_wall_dictionary.
- index_wall_dictionary : dictionary with indices for each wall.
- center_frequencies : band center frequencies.
- mean_absorption_coefficients_per_frequency.
- t60_s_per_frequency.
"""


class Room:
    """A room given by volume, surface area and either T60 or a mean absorption coefficient (Sabine's formula gives
    the other).  Attributes: volume, area, t60_s, absorption_coefficient, schroeders_frequency (Hz),
    critical_distance_m (omnidirectional source)."""

    def __init__(self, volume_m3: float, area_m2: float, t60_s: float | None = None,
                 absorption_coefficient: float | None = None):
        assert area_m2 > 0, "Room surface area has to be positive"
        self.volume = volume_m3
        self.area = area_m2
        if t60_s is None:
            assert absorption_coefficient is not None, "Absorption coefficient should not be None"
            assert absorption_coefficient > 0 and absorption_coefficient <= 1, "Absorption coefficient should be ]0, 1]"
            self.absorption_coefficient = absorption_coefficient
            self.t60_s = 0.161 * self.volume / self.area / self.absorption_coefficient
        if absorption_coefficient is None:
            assert t60_s is not None, "T60 should not be None"
            absorption_coefficient = 0.161 * self.volume / self.area / t60_s
            assert absorption_coefficient > 0 and absorption_coefficient <= 1, (
                "Given reverberation time is not valid. Absorption coefficient should be ]0, 1] and not "
                f"{absorption_coefficient}")
            self.t60_s = t60_s
            self.absorption_coefficient = absorption_coefficient
        self.schroeders_frequency = 2000 * np.sqrt(self.t60_s / self.volume)
        self.critical_distance_m = 0.057 * np.sqrt(self.volume / self.t60_s)

    @property
    def volume(self):
        return self.__volume

    @volume.setter
    def volume(self, new_volume):
        assert new_volume > 0, "Room volume has to be positive"
        self.__volume = new_volume

    @property
    def area(self):
        return self.__area

    @area.setter
    def area(self, new_area):
        assert new_area > 0, "Room volume has to be positive"  # (the reference's message)
        self.__area = new_area

    def modal_density(self, f_hz, c: float = 343):
        """Modes per Hz at f_hz: 4 pi f^2 V / c^3 + pi f S / (2 c^2)."""
        return 4 * np.pi * f_hz ** 2 * self.volume / c ** 3 + np.pi * f_hz * self.area / 2 / c ** 2


class ShoeboxRoom(Room):
    """A rectangular room with one corner at the origin.  dimensions_m: (x, y, z)."""

    def __init__(self, dimensions_m, t60_s: float | None = None, absorption_coefficient: float | None = None):
        dimensions_m = np.atleast_1d(np.squeeze(dimensions_m))
        assert len(dimensions_m) == 3, "Dimensions for a shoebox room should have length 3 (x, y, z)"
        assert np.all(dimensions_m > 0), "Room dimensions must be positive"
        self.dimensions_m = dimensions_m
        super().__init__(np.prod(dimensions_m), np.roll(dimensions_m, 1) @ dimensions_m * 2, t60_s,
                         absorption_coefficient)

    def check_if_in_room(self, coordinates_m) -> bool:
        """True when no coordinate exceeds the room's dimension (only the upper side is tested, as in the reference)."""
        return bool(np.all(np.squeeze(coordinates_m) <= self.dimensions_m))

    def get_mixing_time(self, mode: str = "perceptual", n_reflections: int = 400, c: float = 343) -> float:
        """The time where late reverberation starts: 'perceptual' (Lindau et al. 2012, eq. 13) or 'physical' (the time
        at which the reflection density reaches n_reflections).  Kept in mixing_time_s."""
        mode = mode.lower()
        assert mode in ("perceptual", "physical"), f"{mode} is not supported. Use perceptual or physical"
        if mode == "perceptual":
            mixing_time_s = (np.sqrt(self.volume) * 0.58 + 21.2) * 1e-3
        else:
            assert n_reflections > 0, "n_reflections must be positive"
            mixing_time_s = np.sqrt(n_reflections * self.volume / (4 * np.pi * c ** 3))
        self.mixing_time_s = mixing_time_s
        return self.mixing_time_s

    def _mode_orders(self, max_order: int) -> np.ndarray:
        """(nx, ny, nz) of every mode up to max_order per axis, nx slowest, without (0, 0, 0): the reference's loops."""
        n = np.arange(max_order + 1)
        return np.stack(np.meshgrid(n, n, n, indexing="ij"), axis=-1).reshape(-1, 3)[1:]

    def get_room_modes(self, max_order: int = 6, c: float = 343.0) -> np.ndarray:
        """Modes of the hard-walled room, sorted by frequency: rows (frequency in Hz, nx, ny, nz).  Kept in modes_hz."""
        orders = self._mode_orders(max_order)
        q = (orders / self.dimensions_m) ** 2
        freq = c / 2 * np.sqrt(q[:, 0] + q[:, 1] + q[:, 2])
        modes = np.concatenate([freq[:, None], orders], axis=1)
        self.modes_hz = modes[modes[:, 0].argsort()]
        return self.modes_hz

    def get_analytical_transfer_function(self, source_pos, receiver_pos, freqs, max_mode_order: int = 10,
                                         generate_plot: bool = True, c: float = 343):
        """The modal sum p(f) = 8 c^2 / V sum_n prod(cos(k_n s) cos(k_n r)) / (cn (omega_n^2 + 2j eta_n omega_n -
        omega^2)) over the modes up to max_mode_order per axis, on the device.  eta_n = ln(1000) / T60, with
        detailed absorption the T60 of the octave band nearest to the mode.  Returns (p, modes sorted by frequency,
        None); plots are not built: generate_plot=True, the reference's default, raises NotImplementedError."""
        if generate_plot:
            raise NotImplementedError("get_analytical_transfer_function: plotting is not built; pass generate_plot=False")
        source_pos = np.asarray(source_pos).squeeze()
        receiver_pos = np.asarray(receiver_pos).squeeze()
        assert self.check_if_in_room(source_pos), "Given source position is not in the room"
        assert self.check_if_in_room(receiver_pos), "Given receiver position is not in the room"
        omega = 2 * np.pi * np.asarray(freqs).squeeze()
        orders = self._mode_orders(max_mode_order)
        ks = orders / self.dimensions_m * np.pi
        omega_n = c * np.sqrt((ks[:, None, :] @ ks[:, :, None])[:, 0, 0])  # the reference's ks @ ks, mode by mode
        mode_freq = omega_n / 2 / np.pi
        if hasattr(self, "detailed_absorption"):
            damping = np.log(1e3) / self.detailed_absorption["t60_s_per_frequency"]
            bands = self.detailed_absorption["center_frequencies"]
            eta = damping[np.argmin(np.abs(mode_freq[:, None] - bands[None, :]), axis=1)]
        else:
            eta = np.full(len(omega_n), np.log(1e3) / self.t60_s)
        cn = np.array([4, 2, 1])[np.sum(orders.astype(bool), axis=1) - 1]  # axial, tangential, oblique
        shape = np.cos(ks * source_pos) * np.cos(ks * receiver_pos)
        weight = (shape[:, 0] * shape[:, 1]) * shape[:, 2] / cn
        p = backend.room_modal_response(omega_n, eta, weight, np.atleast_1d(omega ** 2))
        p *= 8 * c ** 2 / np.prod(self.dimensions_m)
        modes = np.concatenate([mode_freq[:, None], orders], axis=1)
        return p, modes[modes[:, 0].argsort()], None

    def add_detailed_absorption(self, detailed_absorption: dict):
        """Absorption per wall ('north', 'south', 'east', 'west', 'floor', 'ceiling'; south, west and floor touch the
        origin) in up to 8 octave bands from 125 Hz.  One value is that wall's coefficient in every band; a shorter
        list than the longest one is continued with its last value.  Updates t60_s and absorption_coefficient (a
        mean over the bands with weights 2^band) and keeps everything in self.detailed_absorption."""
        assert len(detailed_absorption) == 6, \
            "The detailed absorption dictionary must have 6 entries (for each wall)"
        walls = set(_WALLS)
        assert walls == set(detailed_absorption.keys()), (
            f"Keys of dictionary: {set(detailed_absorption.keys())}\ndo not match with the necessary keys: {walls}")
        number_of_bands = 1
        for wall in detailed_absorption:
            ab = np.atleast_1d(detailed_absorption[wall])
            if len(ab) == 1:
                detailed_absorption[wall] = ab * np.ones(8)
            elif len(ab) <= 8:
                detailed_absorption[wall] = ab
                number_of_bands = max(number_of_bands, len(ab))
            else:
                raise ValueError("The absorption coefficient must be passed with either 1 or less than 8 coefficients")
            assert np.all(ab < 1) and np.all(ab > 0), "Absorption must be between 0 and 1 (exclusively)"
        absorption_matrix = np.zeros((6, number_of_bands))
        for wall in detailed_absorption:
            ab = detailed_absorption[wall][:number_of_bands]
            ab = np.pad(ab, (0, number_of_bands - len(ab)), "edge")
            detailed_absorption[wall] = ab
            absorption_matrix[_WALLS[wall]] = ab
        dx, dy, dz = self.dimensions_m
        absorption_area = np.zeros(number_of_bands)
        absorption_area += dx * dy * (absorption_matrix[_WALLS["ceiling"]] + absorption_matrix[_WALLS["floor"]])
        absorption_area += dx * dz * (absorption_matrix[_WALLS["south"]] + absorption_matrix[_WALLS["north"]])
        absorption_area += dy * dz * (absorption_matrix[_WALLS["east"]] + absorption_matrix[_WALLS["west"]])
        self.detailed_absorption = detailed_absorption
        self.detailed_absorption["absorption_matrix"] = absorption_matrix
        self.detailed_absorption["absorption_area"] = absorption_area
        self.detailed_absorption["mean_absorption_coefficients_per_frequency"] = mean = absorption_area / self.area
        self.detailed_absorption["center_frequencies"] = 125 * 2 ** np.arange(number_of_bands)
        self.detailed_absorption["t60_s_per_frequency"] = 0.161 * self.volume / absorption_area
        self.detailed_absorption["index_wall_dictionary"] = dict(_WALLS)
        self.detailed_absorption["README"] = _README
        weights = 2.0 ** np.arange(number_of_bands)
        weights /= np.sum(weights)
        self.absorption_coefficient = np.sum(mean * weights)
        self.t60_s = 0.161 * self.volume / (self.absorption_coefficient * self.area)
