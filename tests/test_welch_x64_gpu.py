"""The float64 Welch entries of the C ABI (ds_welch_spec_x64, ds_welch_tf_x64, ds_csm_x64) against a long-double oracle, at
a bound of four times what a float64 emulation achieves on the CPU: the route matrix of tests/x64_cases.py, one case per
edge of the kernels in csrc/kernels_welch_f64.hpp.  Every case asserts the kernels that ran and prints its worst
error / bound."""

import numpy as np
import pytest

import x64_cases as xc
from dsptoolbox_amd import backend

pytestmark = pytest.mark.gpu


def _call(ctx, p, entry):
    """one call of the entry the case names, through ctx.lib -> the arrays it wrote"""
    B, n, W, hop, F = p["W"] // 2 + 1, p["n"], p["W"], p["hop"], p["n_frames"]
    avg = backend.DS_AVG[p["average"]]
    x, y, w = p["x"], p["y"], p["w"]
    tail = (p["amp_sqrt"], p["norm_scale"], p["factor"], p["halve_edges"])
    kind = entry.split(":")[0]
    if kind == "tf":
        tf, coh = np.zeros((B, p["n_cy"]), np.complex128), np.zeros((B, p["n_cy"]), np.float64)
        ctx.check(ctx.lib.ds_welch_tf_x64(ctx.handle, x.ctypes.data, p["n_cx"], y.ctypes.data, p["n_cy"], n, W, hop, F,
                                          w.ctypes.data, p["detrend"], avg, backend.DS_TF[entry[3:]], *tail, tf.ctypes.data,
                                          coh.ctypes.data), "ds_welch_tf_x64")
        return tf, coh
    if kind == "csm":
        out = np.zeros((B, p["n_cx"], p["n_cx"]), np.complex128)
        ctx.check(ctx.lib.ds_csm_x64(ctx.handle, x.ctypes.data, p["n_cx"], n, W, hop, F, w.ctypes.data, p["detrend"], avg, *tail,
                                     out.ctypes.data), "ds_csm_x64")
        return out
    out = np.zeros((B, p["n_cx"]), np.complex128)
    ctx.check(ctx.lib.ds_welch_spec_x64(ctx.handle, x.ctypes.data, y.ctypes.data if kind == "csd" else None, p["n_cx"], n, W, hop,
                                        F, w.ctypes.data, p["detrend"], avg, *tail, out.ctypes.data), "ds_welch_spec_x64")
    return out


@pytest.mark.parametrize("ident", xc.IDENTS)
def test_float64_welch_route_matrix(ident):
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    p = xc.problem(ident)
    failed = []
    for entry in p["entries"]:
        ctx.routes()
        out = _call(ctx, p, entry)
        assert ctx.routes() == xc.routes(p, entry), (ident, entry)
        try:
            worst = xc.judge_entry(p, entry, out)
        except AssertionError as e:  # (judge every entry of the case before failing it)
            failed.append(e)
            print(f"x64 {ident} {entry}: FAILED {e}")
            continue
        print(f"x64 {ident} {entry}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
              + f" (bound {xc.tolerance(xc.tol_key(p, entry)):.3g})")
    assert not failed, failed
