"""Oracles of the shoebox room simulation, written from the behaviour of the reference (room_acoustics/
_room_acoustics.py:162-269 and :554-685), not from the device code.

ism_oracle: a vectorised float64 restatement of the image-source loop -- the reference's statements in the reference's
order, one plane of l at a time; inside a cell a source whose sample index equals that of a later source of the cell is
dropped (the reference's fancy-index += keeps the last one), across cells np.add.at adds in loop order.  Besides the
response it returns the number of terms per bin (the k of the tests' bound 4 k eps) and the smallest distance of any
source's d / c sr + 0.5 from an integer (the tests' index-exactness premise).

modal_oracle: the modal sum in long double from the same float64 table the device gets, and sum |term| per bin."""

import numpy as np

U = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0], [1, 1, 1]])
EPS = np.finfo(np.float64).eps


def ism_limit(room_dim, t60, max_order, c=343):
    l_max = c * (t60 * 1.1) / 2 / np.asarray(room_dim, dtype=np.float64)
    limit = int(np.ceil(np.sqrt(l_max @ l_max)))
    if max_order is not None:
        limit = limit if max_order > limit else max_order
    return limit


def ism_betas(alpha):
    beta = np.atleast_1d(np.sqrt(1 - np.asarray(alpha, dtype=np.float64)))
    if len(beta) == 1:
        return np.ones(3) * beta, np.ones(3) * beta
    return np.array([beta[1], beta[3], beta[4]]), np.array([beta[0], beta[2], beta[5]])  # south west floor | north east ceiling


def ism_oracle(room_dim, alpha, s_pos, r_pos, t60, max_order, sr, n_out=None, c=343):
    """(rir[n_out], terms per bin, overwritten sources, sources, min distance of an index argument from an integer).
    n_out None: the reference's buffer, int(1.1 t60 5 sr).  IndexError beyond that buffer, as in the reference."""
    room_dim, s_pos, r_pos = (np.asarray(v, dtype=np.float64) for v in (room_dim, s_pos, r_pos))
    beta_1, beta_2 = ism_betas(alpha)
    limit = ism_limit(room_dim, t60, max_order, c)
    buffer_length = int(t60 * 1.1 * 5 * sr)
    n_out = buffer_length if n_out is None else n_out
    rir, terms = np.zeros(n_out), np.zeros(n_out, dtype=np.int64)
    axis = np.arange(-limit, limit + 1)
    m, n = (g.ravel() for g in np.meshgrid(axis, axis, indexing="ij"))
    overwritten, margin = 0, np.inf
    for l in axis:
        lvec = np.stack([np.full_like(m, l), m, n], axis=1)                       # (cells, 3), loop order
        pos = ((1 - 2 * U)[None] * s_pos) + (2 * lvec * room_dim)[:, None, :] - r_pos  # (cells, 8, 3)
        sq = pos ** 2
        d = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) ** 0.5
        arg = d / c * sr + 0.5
        margin = min(margin, np.abs(arg - np.round(arg)).min())
        idx = arg.astype(np.int64)
        if idx.max() >= buffer_length:
            raise IndexError(f"index {idx.max()} is out of bounds for axis 0 with size {buffer_length}")
        k1 = np.abs(lvec[:, None, :] - U[None])
        b1 = beta_1 ** k1
        b2 = beta_2 ** np.abs(lvec)
        damping = ((b1[..., 0] * b1[..., 1]) * b1[..., 2]) * ((b2[:, 0] * b2[:, 1]) * b2[:, 2])[:, None]
        value = damping / (4 * np.pi * d)
        kept = np.ones(idx.shape, dtype=bool)
        for u in range(8):
            for v in range(u + 1, 8):
                kept[:, u] &= idx[:, u] != idx[:, v]
        overwritten += int((~kept).sum())
        kept &= idx < n_out
        np.add.at(rir, idx[kept], value[kept])      # row-major over (cell, u): the loop order
        np.add.at(terms, idx[kept], 1)
    return rir, terms, overwritten, 8 * len(axis) ** 3, margin


def modal_table(dimensions, source_pos, receiver_pos, max_mode_order, t60=None, band_t60=None, band_centres=None, c=343):
    """(omega_n, eta, weight, orders) of the modes in the reference's loop order, float64."""
    dimensions = np.asarray(dimensions, dtype=np.float64)
    n = np.arange(max_mode_order + 1)
    orders = np.stack(np.meshgrid(n, n, n, indexing="ij"), axis=-1).reshape(-1, 3)[1:]
    ks = orders / dimensions * np.pi
    omega_n = c * np.sqrt((ks[:, 0] * ks[:, 0] + ks[:, 1] * ks[:, 1]) + ks[:, 2] * ks[:, 2])
    if band_t60 is None:
        eta = np.full(len(omega_n), np.log(1e3) / t60)
    else:
        nearest = np.argmin(np.abs((omega_n / 2 / np.pi)[:, None] - np.asarray(band_centres)[None]), axis=1)
        eta = (np.log(1e3) / np.asarray(band_t60))[nearest]
    cn = np.array([4, 2, 1])[np.sum(orders.astype(bool), axis=1) - 1]
    shape = np.cos(ks * np.asarray(source_pos)) * np.cos(ks * np.asarray(receiver_pos))
    return omega_n, eta, (shape[:, 0] * shape[:, 1]) * shape[:, 2] / cn, orders


def modal_oracle(omega_n, eta, weight, omega2):
    """(p, sum_n |term_n|) per frequency in long double; the inputs are the float64 values the device gets."""
    on = np.asarray(omega_n, dtype=np.longdouble)[:, None]
    et = np.asarray(eta, dtype=np.longdouble)[:, None]
    w = np.asarray(weight, dtype=np.longdouble)[:, None]
    w2 = np.asarray(omega2, dtype=np.longdouble)[None, :]
    den = (on * on - w2) + 1j * (2 * et * on)
    term = w / den
    return term.sum(axis=0), np.abs(term).sum(axis=0)
