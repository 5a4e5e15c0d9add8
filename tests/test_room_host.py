"""Shoebox room simulation without a GPU.  The float64 restatement of the image-source loop (tests/room_oracle.py) is
held to what the reference's own loop produced (tests/golden/room/cases.npz, made by tools/gen_golden_room.py): the
same set of non-zero samples and every sample within 4 k eps of it, k the number of sources in the sample -- the bound
the device is held to against the oracle.  Then the host arithmetic of Room / ShoeboxRoom and the crossover designs
against the reference's values, the new names, and every guard of the Python layer and of the C entries, all of
which answer before any device is touched."""

import ctypes as C
import os
import warnings

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import SIGNATURES, load_library
from dsptoolbox_amd.filterbanks import LRFilterBank, linkwitz_riley_crossovers
from dsptoolbox_amd.room_acoustics import Room, ShoeboxRoom, generate_synthetic_rir
import room_cases as rc
import room_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def golden(which=rc.GOLDEN):
    if which not in _cache:
        z = np.load(os.path.join(ROOT, *which), allow_pickle=False)
        _cache[which] = {k: z[k] for k in z.files}
    return _cache[which]


def test_new_names_exist():
    for name in ("Room", "ShoeboxRoom", "generate_synthetic_rir", "convolve_rir_on_signal"):
        assert name in dsp.room_acoustics.__all__ and hasattr(dsp.room_acoustics, name)
    assert "linkwitz_riley_crossovers" in dsp.filterbanks.__all__
    assert callable(backend.image_source_rir) and callable(backend.room_modal_response)
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()
    lib = load_library()
    for name in ("ds_room_ism", "ds_room_modal_tf"):
        assert f"int {name}(" in header and name in SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("name", list(rc.ISM_CASES))
def test_oracle_reproduces_the_reference(name, capsys):
    z = golden()
    rir, terms, replaced, sources = rc.ism_expected(name)
    if name in rc.ISM_COUNTS:
        want_sources, want_replaced = rc.ISM_COUNTS[name]
        assert sources == want_sources and (want_replaced is None or replaced == want_replaced)
    n = int(z["ism_large_n"]) if name == "large" else len(rir)
    ref = np.zeros(n)
    ref[z[f"ism_{name}_idx"]] = z[f"ism_{name}_val"]
    mine = rir[:n]
    assert np.array_equal(mine != 0, ref != 0)
    hit = ref != 0
    ratio = np.abs(mine[hit] - ref[hit]) / (4 * terms[:n][hit] * room_oracle.EPS * ref[hit])
    with capsys.disabled():
        print(f"\n{name}: {int(hit.sum())} bins, worst |oracle - reference| / (4 k eps reference) = {ratio.max():.3g}")
    assert ratio.max() <= 1.0


def test_short_case_cuts_between_two_occupied_bins():
    full = rc.ism_expected("walls")[0]
    n_out = rc.ISM_CASES["short"]["n_out"]
    assert full[n_out - 1] != 0 and full[n_out] != 0
    assert np.array_equal(rc.ism_expected("short")[0], full[:n_out])
    assert rc.ISM_CASES["long"]["n_out"] > len(full) and not rc.ism_expected("long")[0][len(full):].any()


def test_without_the_in_cell_rule_the_cube_is_wrong():
    """The premise of the cube case: adding the sources a cell's later sources replace changes the peak region by
    more than half the peak, so a device sum that ignores the rule cannot pass."""
    c = rc.ISM_CASES["cube"]
    rir = rc.ism_expected("cube")[0]
    limit = room_oracle.ism_limit(c["dim"], c["t60"], c["max_order"])
    axis = np.arange(-limit, limit + 1)
    lvec = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 1, 3)
    pos = (1 - 2 * room_oracle.U)[None] * np.array(c["s"]) + 2 * lvec * np.array(c["dim"]) - np.array(c["r"])
    d = np.sqrt((pos ** 2).sum(-1))
    beta = np.sqrt(1 - c["alpha"])
    value = beta ** (np.abs(lvec - room_oracle.U[None]).sum(-1) + np.abs(lvec).sum(-1)) / (4 * np.pi * d)
    plain = np.zeros_like(rir)
    np.add.at(plain, (d / 343 * c["sr"] + 0.5).astype(int), value)
    assert np.abs(plain - rir).max() > 0.5 * rir.max()


def test_room_attributes_against_the_reference():
    z = golden()

    def values(r):
        return np.array([r.volume, r.area, r.t60_s, r.absorption_coefficient, r.schroeders_frequency,
                         r.critical_distance_m])

    by_t60 = ShoeboxRoom((5, 4, 3), t60_s=0.5)
    np.testing.assert_allclose(values(by_t60), z["room_by_t60"], rtol=1e-15)
    np.testing.assert_allclose(values(ShoeboxRoom((5, 4, 3), absorption_coefficient=0.2)), z["room_by_alpha"], rtol=1e-15)
    mixing = [by_t60.get_mixing_time("perceptual"), by_t60.get_mixing_time("physical", 1000)]
    np.testing.assert_allclose(mixing, z["room_mixing"], rtol=1e-15)
    assert by_t60.mixing_time_s == mixing[1]
    np.testing.assert_allclose(by_t60.modal_density(np.array([50.0, 200.0, 1000.0])), z["room_modal_density"], rtol=1e-15)
    modes = by_t60.get_room_modes(6)
    assert modes.shape == z["room_modes"].shape == (7 ** 3 - 1, 4)
    assert np.array_equal(modes, z["room_modes"]) and modes is by_t60.modes_hz
    assert by_t60.check_if_in_room([5, 4, 3]) and not by_t60.check_if_in_room([5.1, 1, 1])
    assert by_t60.check_if_in_room([-1, 1, 1])  # only the upper side is tested, as in the reference


@pytest.mark.parametrize("name", list(rc.ABSORPTION_SETS))
def test_detailed_absorption_against_the_reference(name):
    z = golden()
    room = ShoeboxRoom((5, 4, 3), t60_s=0.5)
    room.add_detailed_absorption({k: v for k, v in rc.ABSORPTION_SETS[name].items()})
    d = room.detailed_absorption
    for key, mine in (("matrix", d["absorption_matrix"]), ("area", d["absorption_area"]),
                      ("mean", d["mean_absorption_coefficients_per_frequency"]), ("t60s", d["t60_s_per_frequency"]),
                      ("centres", d["center_frequencies"]), ("alpha", room.absorption_coefficient), ("t60", room.t60_s)):
        want = z[f"absorption_{name}_{key}"]
        assert np.shape(mine) == want.shape
        np.testing.assert_allclose(mine, want, rtol=1e-15)
    assert d["index_wall_dictionary"]["ceiling"] == 5 and "README" in d


def test_room_assertions_and_messages():
    with pytest.raises(AssertionError, match="Room surface area has to be positive"):
        Room(10, 0, t60_s=1)
    with pytest.raises(AssertionError, match="Room volume has to be positive"):
        Room(-1, 10, t60_s=1)
    with pytest.raises(AssertionError, match="Absorption coefficient should not be None"):
        Room(10, 10)
    with pytest.raises(AssertionError, match=r"Absorption coefficient should be \]0, 1\]"):
        Room(10, 10, absorption_coefficient=1.5)
    with pytest.raises(AssertionError, match="Given reverberation time is not valid"):
        Room(1000, 10, t60_s=0.1)
    with pytest.raises(AssertionError, match="should have length 3"):
        ShoeboxRoom((1, 2))
    with pytest.raises(AssertionError, match="Room dimensions must be positive"):
        ShoeboxRoom((1, 2, -3), t60_s=0.1)
    room = ShoeboxRoom((5, 4, 3), t60_s=0.5)
    with pytest.raises(AssertionError, match="is not supported. Use perceptual or physical"):
        room.get_mixing_time("other")
    with pytest.raises(AssertionError, match="must have 6 entries"):
        room.add_detailed_absorption(dict(north=0.1))
    with pytest.raises(AssertionError, match="do not match with the necessary keys"):
        room.add_detailed_absorption(dict(north=0.1, south=0.1, east=0.1, west=0.1, floor=0.1, roof=0.1))
    with pytest.raises(ValueError, match="either 1 or less than 8"):
        room.add_detailed_absorption(dict(north=[0.1] * 9, south=0.1, east=0.1, west=0.1, floor=0.1, ceiling=0.1))
    with pytest.raises(AssertionError, match="between 0 and 1"):
        room.add_detailed_absorption(dict(north=1.0, south=0.1, east=0.1, west=0.1, floor=0.1, ceiling=0.1))
    with pytest.raises(NotImplementedError, match="plotting is not built"):
        room.get_analytical_transfer_function([1, 1, 1], [2, 2, 2], [100.0])
    with pytest.raises(AssertionError, match="Given source position is not in the room"):
        room.get_analytical_transfer_function([6, 1, 1], [2, 2, 2], [100.0], generate_plot=False)
    with pytest.raises(AssertionError, match="Room must be of type ShoeboxRoom"):
        generate_synthetic_rir(Room(60, 94, t60_s=0.5), [1, 1, 1], [2, 2, 2], 8000)
    with pytest.raises(AssertionError, match="Receiver is not located inside the room"):
        generate_synthetic_rir(room, [1, 1, 1], [2, 2, 9], 8000)
    with pytest.raises(AssertionError, match="no detailed absorption dictionary"):
        generate_synthetic_rir(room, [1, 1, 1], [2, 2, 2], 8000, use_detailed_absorption=True)


def test_image_source_guards_answer_on_the_host():
    args = dict(s_pos=[1, 1, 1], r_pos=[2, 2, 2], t60_s=0.3, max_order=None, sr=8000, n_out=100)
    # the reference's IndexError in an elongated room: int(1.1 * 0.3 * 5 * 8000) = 13200 samples
    with pytest.raises(IndexError, match=r"index \d+ is out of bounds for axis 0 with size 13200"):
        backend.image_source_rir([20, 3, 3], [0.25], **args)
    with pytest.raises(IndexError):
        room_oracle.ism_oracle([20, 3, 3], 0.25, [1, 1, 1], [2, 2, 2], 0.3, None, 8000)
    with pytest.raises(IndexError):
        generate_synthetic_rir(ShoeboxRoom((20, 3, 3), t60_s=0.3), [1, 1, 1], [2, 2, 2], 8000)
    with pytest.raises(ValueError, match="coincide"):
        backend.image_source_rir([5, 4, 3], [0.25], **dict(args, r_pos=[1, 1, 1]))
    with pytest.raises(ValueError, match="Wrong length for absorption coefficients"):
        backend.image_source_rir([5, 4, 3], [[0.2, 0.3]], **args)
    with pytest.raises(NotImplementedError, match=str(backend.ISM_MAX_CELLS)):
        backend.image_source_rir([0.5, 0.5, 0.5], [0.01], **dict(args, t60_s=1.5, sr=1000))  # LIMIT = 981
    with pytest.raises(NotImplementedError, match=str(backend.ISM_MAX_OUT)):
        backend.image_source_rir([5, 4, 3], [0.25], **dict(args, n_out=backend.ISM_MAX_OUT + 1))
    with pytest.raises(NotImplementedError, match=f"{backend.ISM_MAX_BANDS} bands"):
        backend.image_source_rir([5, 4, 3], np.full((9, 1), 0.25), **args)
    with pytest.raises(NotImplementedError, match="does not hold one plane"):
        backend.image_source_rir([5, 4, 3], [0.25], **dict(args, max_list_bytes=1000))
    with pytest.raises(NotImplementedError, match="work bound"):
        backend.room_modal_response(np.ones(10 ** 6), np.ones(10 ** 6), np.ones(10 ** 6), np.ones(10 ** 5 + 1))
    assert backend.ism_limit([5, 4, 3], 0.5, None) == 44 and backend.ism_limit([10, 8, 4], 2.0, None) == 113
    assert backend.ism_limit([5, 4, 3], 0.5, 7) == 7 and backend.ism_limit([5, 4, 3], 0.5, 100) == 44


def test_python_bounds_are_the_sources():
    guards = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "size_guards.hpp")).read()
    assert f"kIsmMaxCells = (int64_t)1 << {backend.ISM_MAX_CELLS.bit_length() - 1};" in guards
    assert f"kIsmMaxListBytes = (int64_t)1 << {backend.ISM_MAX_LIST_BYTES.bit_length() - 1};" in guards
    assert f"kIsmMaxOut = (int64_t)1 << {backend.ISM_MAX_OUT.bit_length() - 1};" in guards
    assert f"kIsmMaxBands = {backend.ISM_MAX_BANDS};" in guards
    assert f"kModalMaxWork = {backend.MODAL_MAX_WORK:.0e}".replace("e+", "e") in guards


def test_c_entries_check_before_touching_a_device():
    lib = load_library()
    v3 = (C.c_double * 3)(5.0, 4.0, 3.0)
    buf = (C.c_double * 64)()
    ism = lib.ds_room_ism
    assert ism(None, v3, v3, v3, 8000.0, 343.0, 1, buf, 1, 8, 0, buf) == -1                    # DS_ERR_ARG: null context
    assert ism(None, v3, v3, v3, 8000.0, 343.0, 1, None, 1, 8, 0, buf) == -1                   # no table
    modal = lib.ds_room_modal_tf
    assert modal(None, buf, buf, buf, 0, buf, 8, buf) == -1                                     # no mode
    assert modal(None, buf, buf, buf, 10 ** 6, buf, 10 ** 5 + 1, buf) == -2                     # DS_ERR_UNSUP: work bound


def wall_powers_rows():
    return backend._ism_wall_powers([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], 3)


def test_wall_power_table_layout():
    pw = wall_powers_rows()
    beta = np.sqrt(1 - np.array([0.2, 0.4, 0.5, 0.1, 0.3, 0.6]))  # south west floor | north east ceiling
    assert pw.shape == (6, 5)
    for k in range(5):
        assert np.array_equal(pw[:, k], beta ** k)
    assert np.array_equal(backend._ism_wall_powers(0.25, 2), np.sqrt(0.75) ** np.arange(4)[None, :] * np.ones((6, 1)))


@pytest.mark.parametrize("name", list(rc.SOS_CASES))
def test_crossover_sections_against_the_reference(name):
    z = golden(rc.GOLDEN_CROSSOVER)
    order, f0, fs = rc.SOS_CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # odd orders warn
        fb = linkwitz_riley_crossovers([f0], order, fs)
    assert isinstance(fb, LRFilterBank) and fb.number_of_bands == 2
    for mine, want in zip(fb.sos[0], (z[f"sos_{name}_lp"], z[f"sos_{name}_hp"])):
        assert mine.shape == want.shape
        np.testing.assert_allclose(mine, want, rtol=1e-13, atol=1e-300)


def test_crossover_order_rules_and_metadata():
    with pytest.warns(UserWarning, match="recommended to be even"):
        linkwitz_riley_crossovers([1000], 3, 48000)
    with pytest.raises(AssertionError, match="6.0 order is not supported for crossover"):
        linkwitz_riley_crossovers([1000], 6, 48000)
    with pytest.raises(AssertionError, match="above nyquist"):
        linkwitz_riley_crossovers([30000], 4, 48000)
    with pytest.raises(AssertionError, match="do not match"):
        linkwitz_riley_crossovers([100, 1000], [4, 4, 4], 48000)
    fb = linkwitz_riley_crossovers([2000, 500], [4, 8], 48000)
    assert list(fb.freqs) == [500, 2000] and list(fb.order) == [8, 4]  # sorted by frequency, orders follow
    assert fb.number_of_cross == 2 and fb.number_of_bands == 3 and fb.info["number_of_bands"] == 3
    np.testing.assert_allclose(fb.center_frequencies, [250, 1250, 13000])
    assert fb.sos[0][0].shape == (4, 6) and fb.sos[1][0].shape == (2, 6)
    fb.initialize_zi(2)
    splits, allpasses = fb.channels_zi[1]
    assert len(fb.channels_zi) == 2 and len(splits) == 2 and len(allpasses) == 4
    assert allpasses[0] is allpasses[1] and allpasses[2] is allpasses[3]  # the reference's layout: rows repeat
    assert splits[0][0].shape == (4, 2) and allpasses[0][1][1].shape == (2, 2)
    twin = fb.copy()
    twin.sos[0][0][0, 0] = 0.0
    assert fb.sos[0][0][0, 0] != 0.0
    s = dsp.Signal(None, np.zeros((64, 1)), 44100)
    with pytest.raises(AssertionError, match="Sampling rates do not match"):
        fb.filter_signal(s)
