"""Golden vectors for the shoebox room simulation and the Linkwitz-Riley crossover bank, made by RUNNING THE REFERENCE
(dsptoolbox 0.8: room_acoustics._room_acoustics._generate_rir, ShoeboxRoom, room_acoustics.generate_synthetic_rir,
filterbanks.linkwitz_riley_crossovers):  python tools/gen_golden_room.py   (half a minute: the reference's loop)

The inputs are the numbers of tests/room_cases.py.  Writes tests/golden/room/cases.npz:
- ism_<case>_{idx,val}: the non-zero samples of _generate_rir for every case of ISM_CASES, padded or trimmed to the
  case's n_out ('large' keeps its first 16384 samples only: ism_large_n says so);
- rir_<path>: generate_synthetic_rir's time data for the four paths of RIR_PATHS ('noise' under np.random.seed(RIR_SEED));
- room_*: attributes of ShoeboxRoom((5, 4, 3), ...) by Sabine both ways, both mixing times, modal_density,
  get_room_modes(6), and absorption_<set>_{matrix,area,mean,t60s,alpha,t60,centres} per set of ABSORPTION_SETS;
- modal_<order>_{p,modes} and modal_<order>d_{p,modes}: get_analytical_transfer_function on modal_freqs() for every
  order of MODAL_ORDERS without and with the detailed absorption of ABSORPTION_SETS['short'];
and tests/golden/room/crossover.npz:
- sos_<case>_{lp,hp}: the crossover sections of SOS_CASES;
- bank_{plain,zero,zi1,zi2} (bands, 3000, 2) and bank_summed (3000, 2): the bank BANK on bank_signal() -- standard,
  zero_phase, two successive activate_zi calls, and Summed mode."""

import contextlib
import importlib
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
import room_cases as rc  # noqa: E402

LARGE_KEPT = 16384


def stack(multiband):
    return np.stack([b.time_data for b in multiband.bands])


def main():
    warnings.simplefilter("ignore")
    dsp = import_reference()
    ra = dsp.room_acoustics
    inner = importlib.import_module("dsptoolbox.room_acoustics._room_acoustics")
    pad_trim = importlib.import_module("dsptoolbox.helpers.other")._pad_trim
    z = {}
    for name, c in rc.ISM_CASES.items():
        alpha = np.asarray(c["alpha"]) if np.ndim(c["alpha"]) else c["alpha"]
        rir = inner._generate_rir(np.asarray(c["dim"]), alpha, np.asarray(c["s"]), np.asarray(c["r"]), c["t60"],
                                  c["max_order"], c["sr"])
        if c["n_out"] is not None:
            rir = pad_trim(rir, c["n_out"])
        if name == "large":
            rir = rir[:LARGE_KEPT]
            z["ism_large_n"] = np.array(LARGE_KEPT)
        z[f"ism_{name}_idx"] = np.nonzero(rir)[0].astype(np.int32)
        z[f"ism_{name}_val"] = rir[rir != 0]

    q = rc.RIR_ROOM
    for path, switches in rc.RIR_PATHS.items():
        room = ra.ShoeboxRoom(q["dim"], t60_s=q["t60"])
        if switches.get("use_detailed_absorption"):
            room.add_detailed_absorption({k: v for k, v in rc.RIR_DETAILED.items()})
        np.random.seed(rc.RIR_SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            out = ra.generate_synthetic_rir(room, q["s"], q["r"], q["sr"], total_length_seconds=q["length_s"], **switches)
        z[f"rir_{path}"] = out.time_data[:, 0]

    by_t60 = ra.ShoeboxRoom((5, 4, 3), t60_s=0.5)
    by_alpha = ra.ShoeboxRoom((5, 4, 3), absorption_coefficient=0.2)
    z["room_by_t60"] = np.array([by_t60.volume, by_t60.area, by_t60.t60_s, by_t60.absorption_coefficient,
                                 by_t60.schroeders_frequency, by_t60.critical_distance_m])
    z["room_by_alpha"] = np.array([by_alpha.volume, by_alpha.area, by_alpha.t60_s, by_alpha.absorption_coefficient,
                                   by_alpha.schroeders_frequency, by_alpha.critical_distance_m])
    z["room_mixing"] = np.array([by_t60.get_mixing_time("perceptual"), by_t60.get_mixing_time("physical", 1000)])
    z["room_modal_density"] = by_t60.modal_density(np.array([50.0, 200.0, 1000.0]))
    z["room_modes"] = by_t60.get_room_modes(6)
    for name, walls in rc.ABSORPTION_SETS.items():
        room = ra.ShoeboxRoom((5, 4, 3), t60_s=0.5)
        room.add_detailed_absorption({k: v for k, v in walls.items()})
        d = room.detailed_absorption
        z[f"absorption_{name}_matrix"] = d["absorption_matrix"]
        z[f"absorption_{name}_area"] = d["absorption_area"]
        z[f"absorption_{name}_mean"] = d["mean_absorption_coefficients_per_frequency"]
        z[f"absorption_{name}_t60s"] = d["t60_s_per_frequency"]
        z[f"absorption_{name}_centres"] = d["center_frequencies"]
        z[f"absorption_{name}_alpha"] = np.array(room.absorption_coefficient)
        z[f"absorption_{name}_t60"] = np.array(room.t60_s)

    m = rc.MODAL_ROOM
    for order in rc.MODAL_ORDERS:
        for tag in ("", "d"):
            room = ra.ShoeboxRoom(m["dim"], t60_s=m["t60"])
            if tag:
                room.add_detailed_absorption({k: v for k, v in rc.ABSORPTION_SETS["short"].items()})
            p, modes, _ = room.get_analytical_transfer_function(m["s"], m["r"], rc.modal_freqs(), max_mode_order=order,
                                                                generate_plot=False)
            z[f"modal_{order}{tag}_p"], z[f"modal_{order}{tag}_modes"] = p, modes
    write(os.path.join(ROOT, *rc.GOLDEN), z)

    z = {}
    for name, (order, f0, fs) in rc.SOS_CASES.items():
        fb = dsp.filterbanks.linkwitz_riley_crossovers([f0], order, fs)
        z[f"sos_{name}_lp"], z[f"sos_{name}_hp"] = fb.sos[0]
    b = rc.BANK
    sig = dsp.Signal(None, rc.bank_signal(), b["sr"], constrain_amplitude=False)

    def bank():
        return dsp.filterbanks.linkwitz_riley_crossovers(b["freqs"], b["order"], b["sr"])

    z["bank_plain"] = stack(bank().filter_signal(sig))
    z["bank_zero"] = stack(bank().filter_signal(sig, zero_phase=True))
    fb = bank()
    z["bank_zi1"] = stack(fb.filter_signal(sig, activate_zi=True))
    z["bank_zi2"] = stack(fb.filter_signal(sig, activate_zi=True))
    z["bank_summed"] = bank().filter_signal(sig, mode=dsp.FilterBankMode.Summed).time_data
    write(os.path.join(ROOT, *rc.GOLDEN_CROSSOVER), z)


def write(path, z):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()
