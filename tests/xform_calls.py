"""How the tests call the whole-signal rFFT and deconvolution entries of the C-ABI on a problem of route_cases.py or
xform_cases.py: shared by test_gpu_parity.py (the route matrices) and test_xform_sweep_gpu.py, so that both call the
entries the same way."""

import numpy as np


def route_call(ctx, fn, args):
    """(launch names) of one C-ABI call, or ["ERR<code>"] where the call returns an error."""
    rc = fn(ctx.handle, *args)
    return sorted(ctx.routes()) if rc == 0 else [f"ERR{rc}"]


def rfft_route_case(entry, q):
    """One whole-signal spectrum (route_cases.rfft_problem) through one C-ABI entry point -> (output array, launch
    names)."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context
    ctx = get_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    x, xp, n, n_fft, n_ch, B, scale = q["x"], q["xp"], q["n"], q["n_fft"], q["n_ch"], q["B"], C.c_float(q["scale"])
    ctx.routes()
    if entry.endswith("_dev"):
        dx, do = DevicePlanar.from_planar(ctx, xp), DeviceBuffer(ctx, B * n_ch * 8)
        routes = route_call(ctx, ctx.lib.ds_rfft_dev, (C.c_void_p(dx.ptr), n_ch, dx.ld, n, n_fft, scale, C.c_void_p(do.ptr)))
        out = do.to_array((B, n_ch), np.complex64)
        for b in (dx.owner, do):
            b.free()
        return out, routes
    f64 = entry.endswith("_f64")
    out = np.zeros((B, n_ch), np.complex128 if f64 else np.complex64)
    fn = ctx.lib.ds_rfft_f64 if f64 else ctx.lib.ds_rfft
    routes = route_call(ctx, fn, (p(np.ascontiguousarray(x.T) if f64 else xp), n_ch, n, n_fft, scale, p(out)))
    return out, routes


def deconv_route_case(entry, q):
    """One batch of deconvolutions (route_cases.deconv_problem) through one C-ABI entry point -> (output array, launch
    names).  ds_deconv_f64 takes one item."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context
    ctx = get_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    y, yp, r, n, n_fft, n_ch, n_items, r_per_channel, n_out = (q[k] for k in ("y", "yp", "r", "n", "n_fft", "n_ch", "n_items",
                                                                             "r_per_channel", "n_out"))
    ctx.routes()
    if entry.endswith("_dev"):
        dy, dr, do = DevicePlanar.from_planar(ctx, yp), DeviceBuffer.from_array(ctx, r), DeviceBuffer(ctx, yp.shape[0] * n_out * 4)
        routes = route_call(ctx, ctx.lib.ds_deconv_dev, (C.c_void_p(dy.ptr), n_items, n_ch, dy.ld, n, n_fft, C.c_void_p(dr.ptr),
                                                         r_per_channel, n_out, n_out, C.c_void_p(do.ptr)))
        out = do.to_array((n_items, n_ch, n_out), np.float32)
        for b in (dy.owner, dr, do):
            b.free()
        return out, routes
    if entry.endswith("_f64"):
        out = np.zeros((n_out, n_ch), np.float64)
        routes = route_call(ctx, ctx.lib.ds_deconv_f64, (p(np.ascontiguousarray(y.T)), n_ch, n, n_fft, p(r), r_per_channel,
                                                         n_out, p(out)))
        return out, routes
    out = np.zeros((n_items, n_ch, n_out), np.float32)
    routes = route_call(ctx, ctx.lib.ds_deconv, (p(yp), n_items, n_ch, n, n_fft, p(r), r_per_channel, n_out, p(out)))
    return out, routes
