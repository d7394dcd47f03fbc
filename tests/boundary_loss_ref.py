"""Float64 numpy statement of the boundary loss (csrc/boundary_loss.hip, unetseg_boundary_loss_fwd): the
signed distance map phi, the loss L and its gradient gz = dL/dz, as include/unetseg_hip.h defines them.  The
squared distances come from tests/boundary_ref.py (itself held to scipy's exact transform);
tests/test_boundary_loss_cpu.py holds this file to scipy's transform written out as the published
one_hot2dist, to hand-written maps and to PyTorch float64 autograd.
"""
import numpy as np

from boundary_ref import INF, sqdist

U = 2.0 ** -24  # one fp32 rounding, relative


def site_maps(t, c=1, ignore=None):
    """(fg, bg, valid) bool [B,H,W]: fg = {t == c}, bg = {t != c, t != ignore}, valid = not ignored"""
    t = np.asarray(t)
    valid = np.ones(t.shape, bool) if ignore is None else t != ignore
    fg = t == c
    return fg, ~fg & valid, valid


def sq_distances(t, c=1, ignore=None):
    """(d2fg, d2bg) int64 [B,H,W]: exact squared distance to the nearest fg / bg pixel of the same image, INF
    where the image has none"""
    fg, bg, _ = site_maps(t, c, ignore)
    return sqdist(fg).astype(np.int64), sqdist(bg).astype(np.int64)


def signed_distance(t, c=1, ignore=None):
    """phi float64 [B,H,W]: +sqrt(d2fg) on bg, -(sqrt(d2bg) - 1) on fg, 0 on ignored pixels and wherever the
    distance it would use is INF"""
    fg, bg, _ = site_maps(t, c, ignore)
    d2fg, d2bg = sq_distances(t, c, ignore)
    phi = np.zeros(np.asarray(t).shape, np.float64)
    m = bg & (d2fg != INF)
    phi[m] = np.sqrt(d2fg[m].astype(np.float64))
    m = fg & (d2bg != INF)
    phi[m] = -(np.sqrt(d2bg[m].astype(np.float64)) - 1.0)
    return phi


def logit(out):
    """z float64 [B,H,W] of logits [B,2,H,W] (o1 - o0), [B,1,H,W] or [B,H,W]"""
    o = np.asarray(out, np.float64)
    if o.ndim == 3:
        return o
    return o[:, 1] - o[:, 0] if o.shape[1] == 2 else o[:, 0]


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def boundary_loss(out, t, c=1, ignore=None, inv_norm=1.0):
    """(L, gz [B,H,W], phi [B,H,W]) in float64: L = inv_norm / Nvalid * sum_valid p phi, gz = dL/dz;
    L = 0 and gz = 0 without a valid pixel"""
    z = logit(out)
    _, _, valid = site_maps(t, c, ignore)
    phi = signed_distance(t, c, ignore)
    n = int(valid.sum())
    if n == 0:
        return 0.0, np.zeros_like(z), phi
    p = sigmoid(z)
    e = np.exp(-np.abs(z))
    pq = e / (1.0 + e) ** 2  # p (1 - p) without the cancellation of 1 - p
    k = float(inv_norm) / n
    return float(k * (p * phi)[valid].sum()), np.where(valid, pq * phi * k, 0.0), phi


# ---- the error bound of the kernel (derivation: DESIGN.md, "Boundary loss") ------------------------------
K_SIGMOID = 4   # expf, 1 + e and the division: DESIGN.md 4c's asserted bound for the sigmoid, in fp32 ulps
K_PQ = 9        # hi * lo: two such quotients and their product
K_PHI = 2       # the root's half ulp of r is at most r / (r - 1) / 2 <= 1.71 ulps of r - 1 (r >= sqrt 2 on fg)
K_GZ_TAIL = 4   # x phi, the stored inv_norm / Nvalid, x that, x weight


def gz_bound(out, t, gz_ref, nch):
    """per-element bound on |gz - gz_ref|: 1.01 (K_PQ + K_PHI + K_GZ_TAIL + |z| [nch 2: the rounded
    o1 - o0]) U |gz_ref|"""
    zk = np.abs(logit(out)) if nch == 2 else 0.0
    return 1.01 * (K_PQ + K_PHI + K_GZ_TAIL + zk) * U * np.abs(gz_ref)


def loss_bound(out, t, nch, c=1, ignore=None, inv_norm=1.0):
    """bound on |L - L_ref|: every term p phi carries K_SIGMOID + K_PHI + |z| (nch 2) roundings, the
    terms are summed in double, and the result is cast to fp32 once"""
    z = logit(out)
    _, _, valid = site_maps(t, c, ignore)
    n = int(valid.sum())
    if n == 0:
        return 0.0
    L, _, phi = boundary_loss(out, t, c, ignore, inv_norm)
    zk = np.abs(z) if nch == 2 else 0.0
    terms = ((K_SIGMOID + K_PHI + zk) * np.abs(sigmoid(z) * phi))[valid].sum() * float(inv_norm) / n
    return 1.01 * U * (terms + abs(L))
