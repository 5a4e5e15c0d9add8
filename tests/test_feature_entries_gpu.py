"""The host shim of the feature families (csrc/api.hip: beamformer maps, IIR, delay-and-sum, CWT, smoothing, direct DFT,
the float64 FFT family, LPC, ds_fir_freqz) against two tables recorded from the library before these entries were moved
onto one table stager, staged() and one memory pre-check (tools/record_feature_contract.py):

  tests/golden/feature_routes.json    the launches of every accepted call of tests/feature_cases.py
  tests/golden/feature_rejected.json  the code and the full message of every refused one

The messages are compared in full: how they are put together is part of what was rewritten.
"""

import json
import os

import pytest

import feature_cases as fc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _table(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


def test_tables_cover_the_cases():
    """every case has a recorded answer and every answer a case (no GPU needed)"""
    routes = {k + "|again" * i for k, (_, _, times) in fc.ROUTES.items() for i in range(times)}
    assert set(_table("feature_routes.json")) == routes
    assert set(_table("feature_rejected.json")) == set(fc.REJECTED_KEYS)
    # a refused call launched nothing and was not accepted when it was recorded
    assert all(not v.startswith("0|") for v in _table("feature_rejected.json").values())


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(fc.ROUTES))
def test_feature_routes(key):
    table = _table("feature_routes.json")
    seen, _ = fc.run_route(key)
    assert {k: " ".join(v) for k, v in seen.items()} == {k: table[k] for k in seen}


@pytest.mark.gpu
def test_bluestein_tables_are_kept():
    """the second transform of a length in one context does not build the chirp tables again"""
    seen, _ = fc.run_route("ds_fft_c128|12")
    assert "fft64_chirp" in seen["ds_fft_c128|12"] and "fft64_chirp" not in seen["ds_fft_c128|12|again"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", fc.REJECTED_KEYS)
def test_feature_rejected(key):
    from dsptoolbox_amd._lib import get_context
    assert fc.run_rejected(get_context(), key) == _table("feature_rejected.json")[key]
