"""The host shim (dsptoolbox_amd/backend.py) against a recording stand-in for Context, no GPU: which C entry every public
function calls, with which scalar arguments, pointer kinds, allocation sizes, transfers and frees, what it returns (type,
dtype, shape) and what it raises.  tests/golden/backend_calls.json was recorded by tools/record_backend_calls.py before the
shim was rebuilt on one Welch plan, one route function and one device-buffer scope; tests/golden/backend_calls_xform.json
(STFT, iSTFT, rFFT, deconvolution, FIR, beamformer maps, IIR) before that half got one STFT plan and one transport choice
per host function.  The shim must keep reproducing both.  Cases with arrays of 2^20 elements need the built library."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_backend_calls", os.path.join(ROOT, "tools", "record_backend_calls.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)
backend = rec.backend

# The one case whose recorded outcome the rebuilt shim deliberately does not repeat: compute_transfer_function over
# device-resident signals with an overlap of 100 % used to fail inside scipy's check_COLA ("noverlap must be less than
# nperseg.") because the framing ran before any check; an invalid overlap now reaches the host path like an invalid
# window length (its samples come down for it first), and the user sees the reference's assertion.
RESTATED = {"ctf/resident_reject_overlap": {
    "error": ["AssertionError", "overlap_percent should be between 0 and 100"],
    "log": [["malloc", 2048], ["malloc", 4096], ["download", "dev1+0", 4096], ["download", "dev0+0", 2048], ["free", [0, 1]]]}}


@pytest.fixture(scope="module")
def recorded():
    with open(rec.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def transcript():
    return rec.record()


def test_every_welch_entry_is_reached(recorded, transcript):
    for t in (recorded, transcript):
        missing = sorted(set(rec.WELCH_ENTRIES) - rec.entries_reached(t))
        assert not missing, f"no case reaches {missing}"


def test_case_list_matches_the_fixture(recorded, transcript):
    assert sorted(transcript) == sorted(recorded)


@pytest.mark.parametrize("name", sorted(rec.cases()))
def test_call_transcript(name, recorded, transcript):
    want, got = dict(recorded[name]), transcript[name]
    if name in RESTATED:
        assert want["error"] == ["ValueError", "noverlap must be less than nperseg."]
        want.update(RESTATED[name])
    if name.startswith("ctf/") and got["warnings"] != want["warnings"]:
        # the one difference allowed: compute_transfer_function used to compute the framing twice, and so to warn twice
        # about a non-COLA window; one plan warns once
        assert len(want["warnings"]) == 2 and got["warnings"] == sorted(set(want["warnings"]))
        want["warnings"] = got["warnings"]
    assert got == want


# ---- the other half of the shim: STFT, iSTFT, rFFT, deconvolution, FIR, beamformer maps, IIR --------------------------
@pytest.fixture(scope="module")
def recorded_xform():
    with open(rec.FIXTURE_XFORM) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def transcript_xform():
    return rec.record(rec.xform_cases)


def test_every_xform_entry_is_reached(recorded_xform, transcript_xform):
    for t in (recorded_xform, transcript_xform):
        missing = sorted(set(rec.XFORM_ENTRIES) - rec.entries_reached(t))
        assert not missing, f"no case reaches {missing}"


def test_xform_case_list_matches_the_fixture(recorded_xform, transcript_xform):
    assert sorted(transcript_xform) == sorted(recorded_xform)


@pytest.mark.parametrize("name", sorted(rec.xform_cases()))
def test_xform_call_transcript(name, recorded_xform, transcript_xform):
    want, got = dict(recorded_xform[name]), transcript_xform[name]
    if name == "stft/fusable_power_non_cola":
        # the one difference allowed: _stft used to build its plan twice for a large float64 array with a power scaling
        # (once for the fused transport, which such a scaling does not take), and so to warn twice about a non-COLA
        # window; one plan warns once
        assert len(want["warnings"]) == 2 and got["warnings"] == sorted(set(want["warnings"])) and len(got["warnings"]) == 1
        want["warnings"] = got["warnings"]
    assert got == want


# ---- the device-buffer scope ------------------------------------------------------------------------------------------
def test_scope_frees_temporaries_and_keeps_the_result():
    ctx = rec.RecordingContext()
    with backend.device_scope(ctx) as dev:
        a = dev.alloc(100)
        b = dev.upload(np.zeros(7, dtype=np.float32))
        r = dev.alloc(50, result=True)
        assert ctx.live == {0, 1, 2} and (a.nbytes, b.nbytes, r.nbytes) == (100, 28, 50)
    assert ctx.live == {2} and a.ptr is None and b.ptr is None and r.ptr is not None
    assert ctx.free_count == {0: 1, 1: 1}
    r.free()
    assert ctx.live == set() and ctx.free_count == {0: 1, 1: 1, 2: 1}


def test_scope_frees_everything_when_the_body_raises():
    ctx = rec.RecordingContext()
    with pytest.raises(KeyboardInterrupt):
        with backend.device_scope(ctx) as dev:
            dev.alloc(100)
            dev.upload(np.zeros(7))
            r = dev.alloc(50, result=True)
            r.free()  # (a body that let go of a buffer itself: still one free)
            dev.alloc(10, result=True)
            raise KeyboardInterrupt
    assert ctx.live == set() and ctx.free_count == {0: 1, 1: 1, 2: 1, 3: 1}


def test_scope_frees_the_buffer_of_a_failed_upload():
    ctx = rec.RecordingContext()

    def failing_upload(dptr, arr):
        raise RuntimeError("ds_upload failed")
    ctx.upload = failing_upload
    with pytest.raises(RuntimeError, match="ds_upload failed"):
        with backend.device_scope(ctx) as dev:
            dev.upload(np.zeros(3))
    assert ctx.live == set() and ctx.free_count == {0: 1}


def test_scope_leaves_borrowed_memory_alone():
    ctx = rec.RecordingContext()
    w = backend._window_dev(ctx, backend._window_array("hann", 16))
    s = backend._result_scratch(ctx, 10)
    with backend.device_scope(ctx) as dev:
        dev.alloc(8)
    assert ctx.live == {0, 1} and w.ptr is not None and s.ptr is not None
    assert backend._window_dev(ctx, backend._window_array("hann", 16)) is w and backend._result_scratch(ctx, 10) is s


class _FailingCalls:
    """The stand-in's library whose `fail_at`-th entry call (from 1) returns DS_ERR_UNSUP."""

    def __init__(self, ctx, fail_at):
        self._inner, self._left = ctx.lib, fail_at

    def __getattr__(self, name):
        fn = getattr(self._inner, name)

        def entry(*args):
            fn(*args)
            self._left -= 1
            return -2 if self._left == 0 else 0
        return entry


def _failing_context(fail_at):
    ctx = rec.RecordingContext()
    ctx.lib = _FailingCalls(ctx, fail_at)

    def check(rc, what=""):
        if rc != 0:
            raise NotImplementedError(what)
    ctx.check = check
    return ctx


def test_regularized_inverse_leaves_nothing_behind_when_its_call_fails(monkeypatch):
    """Three buffers used to stay allocated until garbage collection when ds_deconv_inverse_dev raised."""
    ctx = _failing_context(1)
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    with pytest.raises(NotImplementedError, match="ds_deconv_inverse"):
        backend.regularized_inverse(np.ones((9, 2), dtype=complex), np.ones(9))
    assert ctx.live == set() and ctx.free_count == {0: 1, 1: 1, 2: 1}


def test_a_failing_second_call_leaves_no_live_allocation(monkeypatch):
    """spectral_division_device makes three calls; regularized_inverse called twice: the second failing."""
    ctx = _failing_context(2)
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    backend.regularized_inverse(np.ones((9, 2), dtype=complex), np.ones(9))
    assert ctx.live == set()
    with pytest.raises(NotImplementedError):
        backend.regularized_inverse(np.ones((9, 2), dtype=complex))
    assert ctx.live == set() and all(v == 1 for v in ctx.free_count.values()) and len(ctx.free_count) == 5
    ctx = _failing_context(2)
    y, x = rec.resident(ctx, 100, 2), rec.resident(ctx, 100, 1)
    with pytest.raises(NotImplementedError, match="ds_deconv_inverse"):
        backend.spectral_division_device(y, x, 128, 120, lambda den: np.ones(den.shape[0]))
    assert ctx.live == {0, 1}  # (the caller's resident samples)
    assert all(v == 1 for v in ctx.free_count.values()) and len(ctx.free_count) == 4


def test_resident_results_are_freed_when_the_call_fails():
    for call in (lambda c: backend._csm_welch_device(rec.resident(c, 100, 2), 48000, 16, "hann", 50.0, True, "mean",
                                                    backend.SpectrumScaling.FFTBackward),
                 lambda c: backend.fir_filter_bank_device(rec.resident(c, 100, 2), [np.ones(5)], backend.DS_FB_PARALLEL),
                 lambda c: backend.cwt_device(rec.resident(c, 100, 2), [0], [np.ones(5, dtype=complex)])):
        ctx = _failing_context(1)
        with pytest.raises(NotImplementedError):
            call(ctx)
        assert ctx.live <= {0} and all(v == 1 for v in ctx.free_count.values())  # (0: the caller's resident samples)
