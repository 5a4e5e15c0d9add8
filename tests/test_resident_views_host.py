"""The views of tests/view_cases.py without a device: the builder lays the samples out as it says, the three views meet
their alignment conditions at every case's length, every resident entry of the header has view cases, and the cases are
small."""

import os
import re

import numpy as np
import pytest

import view_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# input pitches of planar samples, and the flags that say "x is planar float32 on the device"
PITCHES = {"ldx", "ld", "lda", "ldb", "ldxh", "ldy"}
FLAGS = {"on_device", "x_on_device"}
# `_dev` entries whose device operand is not planar samples: outside the view contract
NOT_SAMPLES = (
    ("ds_band_power_dev", "reads a spectrogram (bins, frames x channels), dense by construction"),
    ("ds_das_map_dev", "reads a cross-spectral matrix and steering vectors"),
    ("ds_csm_das_prepare_dev", "reads and writes a cross-spectral matrix"),
    ("ds_bf_eigh_dev", "reads Hermitian matrices, float64"),
    ("ds_bf_eig_map_dev", "reads a cross-spectral matrix and steering vectors, float64"),
    ("ds_bf_cleansc_dev", "reads a cross-spectral matrix and steering vectors, float64"),
    ("ds_istft_dev", "reads a spectrogram; its output pitch is ld_out"),
    ("ds_csm_spec_dev", "reads spectra (bins, frames, channels)"),
    ("ds_deconv_inverse_dev", "reads a spectrum (bins, channels)"),
    ("ds_cwt_squeeze_dev", "reads a scalogram (frequencies, samples, channels)"),
    ("ds_fir_part_step_dev", "a streaming step over the class's own dense buffers"),
    ("ds_fir_ols_step_dev", "a streaming step over the class's own dense buffer row"),
)


def declarations():
    """{entry: [parameter names]} of every function of the header that takes a context."""
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    out = {}
    for name, params in re.findall(r"\bint\s+(ds_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header):
        names = [re.sub(r"\[.*\]", "", p).split()[-1].lstrip("*") for p in params.split(",") if p.strip()]
        if names and names[0] == "ctx":
            out[name] = names
    return out


def resident_entries():
    return {name for name, params in declarations().items() if (PITCHES | FLAGS) & set(params)}


def test_every_resident_entry_has_view_cases():
    decl = declarations()
    assert len(decl) > 80, "the header was not parsed"
    want = resident_entries()
    assert want == set(vc.ENTRIES), sorted(want ^ set(vc.ENTRIES))
    assert all(vc.ENTRIES[name] for name in want)
    outside = {name for name, _ in NOT_SAMPLES}
    assert not outside & want and outside <= set(decl)
    dev = {name for name in decl if name.endswith("_dev")}
    assert dev <= want | outside, sorted(dev - want - outside)  # a new _dev entry is classified one way or the other
    for cases in vc.ENTRIES.values():
        assert len({c.name for c in cases}) == len(cases)


@pytest.mark.parametrize("fill", vc.FILLS)
@pytest.mark.parametrize("n_ch,n", [(1, 1), (3, 7), (2, 4096), (5, 5001)])
def test_layout(n_ch, n, fill):
    x = np.random.default_rng(n).standard_normal((n_ch, n)).astype(np.float32)
    for front, gap in vc.VIEWS(n):
        owner, ld, off = vc.layout(x, front, gap, fill)
        assert owner.dtype == np.float32 and owner.ndim == 1 and ld == n + gap and off == 4 * front
        rows = np.stack([owner[off // 4 + c * ld:off // 4 + c * ld + n] for c in range(n_ch)])
        assert np.array_equal(rows.view(np.uint32), x.view(np.uint32))
        valid = vc.valid_mask(owner.size, n_ch, n, ld, front)
        assert valid.sum() == n_ch * n
        rest = owner[~valid]
        want = vc.poison(owner.size, fill)[~valid]
        assert np.array_equal(rest.view(np.uint32), want.view(np.uint32))
        if fill == "big":
            assert np.all(np.abs(rest) == 2.0 ** 20) and np.all(owner[0::2][~valid[0::2]] > 0) and np.all(owner[1::2][~valid[1::2]] < 0)
        else:
            assert np.all(np.isnan(rest))
        m = max(4096, ld)
        assert front >= m and not valid[:m].any()
        last = front + (n_ch - 1) * ld + n
        assert owner.size - last >= m and not valid[last:].any()


def check_views(n, n_ch):
    (f1, g1), (f2, g2), (f3, g3) = vc.VIEWS(n)
    assert f1 % 4 == 0 and g1 % 4 == 0 and g1 > 0
    assert f2 % 4 == 1 and (n + g2) % 4 == 0
    assert f3 % 4 == 3 and (n + g3) % 2 == 1
    residues = {(f + c * (n + g)) % 4 for f, g in ((f1, g1), (f2, g2), (f3, g3)) for c in range(n_ch)}
    # one row per view gives the residues 0, 1 and 3; the rotating view's second row adds 2
    assert residues == ({0, 1, 2, 3} if n_ch > 1 else {0, 1, 3})


@pytest.mark.parametrize("n", list(range(1, 18)) + [4095, 4096, 4097])
def test_views_at_every_residue_of_n(n):
    check_views(n, 1)
    check_views(n, 2)
    check_views(n, 5)


CASES = vc.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[vc.case_id(c) for c in CASES])
def test_case_inputs(case):
    """float32 planes rebuilt the same from their seeds, views that meet the conditions at the case's lengths, and a
    total input under 16 MB -- 32 MB for a Welch or STFT case on a window above 32768 samples."""
    planes, run = case.build()[:2]
    again = case.build()[0]
    assert callable(run) and len(planes) >= 1
    total = 0
    for p, q in zip(planes, again):
        assert p.dtype == np.float32 and p.ndim == 2 and p.flags.c_contiguous and np.all(np.isfinite(p))
        assert np.array_equal(p, q)
        check_views(p.shape[1], p.shape[0])
        total += p.nbytes
    long_window = re.match(r"(W|nfft)(\d+)_", case.name)
    cap = 32e6 if (long_window and int(long_window.group(2)) > 32768
                   and case.entry in ("ds_welch_tf_dev", "ds_welch_psd_dev", "ds_stft_r2c_dev")) else 16e6
    assert total < cap, (total, cap)


def test_the_windows_cover_every_recorded_launch_name_set():
    """The hot-path cases take one size per distinct set of launch names of the recorded route tables."""
    assert vc.welch_windows("tf") == [32, 2048, 4096, 8192, 16384, 2 ** 20] == vc.welch_windows("psd")
    assert vc.stft_nffts() == [8, 32, 1000, 4096, 8192, 32768, 2 ** 19]
    assert vc.csm_windows("all") == [32, 4096, 16384, 32768] == vc.csm_windows("part")
    assert vc.xform_nffts("rfft") == [3, 8, 32768]
    assert vc.xform_nffts("deconv", 0) == [3, 8, 8192, 32768] and vc.xform_nffts("deconv", 1) == [3, 8, 32768]
    assert vc.fir_taps() == [1, 1025, 4097, 8193]


def test_constants_match_the_families():
    import levels_cases as lc
    from dsptoolbox_amd import backend
    assert vc.FOLLOW_TILE == backend.FX_FOLLOW_TILE
    assert (vc.SPAN, vc.TILE) == (lc.SPAN, lc.TILE) == (backend.LEVEL_SPAN, backend.LEVEL_TILE)
    assert vc.N_RECURSIVE == 2 * 2048 + 1 == backend.PAIR_SPAN + 1
