"""Record what the library answers to the calls of tests/feature_cases.py:

    python tools/record_feature_contract.py [--outputs FILE.npz]

writes tests/golden/feature_routes.json (sorted launch names of every accepted call) and feature_rejected.json
("<code>|<message>" of every refused one).  Run it on the library whose behaviour is the contract -- for a refactor of the
host shim that is the parent commit's, with DSPTOOLBOX_AMD_LIB pointing at it.  --outputs also saves every output array
of the accepted calls, for a bit-for-bit comparison of two libraries (not committed: the bits change with the compiler).
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import feature_cases as fc  # noqa: E402
from dsptoolbox_amd._lib import get_context  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--outputs", help="npz file for the accepted calls' output arrays")
    ap.add_argument("--golden", default=os.path.join(ROOT, "tests", "golden"), help="directory the two tables go to")
    args = ap.parse_args()
    routes, arrays = {}, {}
    for key in fc.ROUTES:
        r, got = fc.run_route(key)
        routes.update({k: " ".join(v) for k, v in r.items()})
        arrays.update({f"{k}|{name}": a for k, outs in got.items() for name, a in outs.items()})
    ctx = get_context()
    rejected = {key: fc.run_rejected(ctx, key) for key in fc.REJECTED_KEYS}
    for name, table in (("feature_routes.json", routes), ("feature_rejected.json", rejected)):
        with open(os.path.join(args.golden, name), "w") as fh:
            json.dump(table, fh, indent=0, sort_keys=True)
            fh.write("\n")
    if args.outputs:
        np.savez(args.outputs, **arrays)
    print(f"{len(routes)} accepted calls, {len(arrays)} output arrays, {len(rejected)} refused calls")


if __name__ == "__main__":
    main()
