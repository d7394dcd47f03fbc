"""Float64 numpy statement of the soft skeleton and the soft-clDice loss (include/unetseg_hip.h, "soft skeleton and
soft-clDice loss"; csrc/cldice.hip), with the stated tie rules, and of the bounds the GPU tests hold.

  E(x)(q) = min over q and its four edge neighbours, window order up, left, centre, right, down
  D(x)(q) = max over the 3 x 3 of q, row-major;  O = D(E(x));  windows clipped to the image
  x_0 = x, s_0 = relu(x_0 - O(x_0));  x_j = E(x_{j-1}), d_j = relu(x_j - O(x_j)), s_j = s_{j-1} + relu(d_j - s_{j-1} d_j)
  relu'(a) = [a > 0]; a window's gradient goes to the first element that attains the extreme in window order

Next to every gradient the backward carries the sum of the absolute values of the terms that enter it (`A`), with
1 - s and 1 - d counted as two terms each (|g| (1 + s), |g| (1 + d)): the bounds are multiples of u = 2^-24 times A.

Rounding counts of the kernels as written (u = 2^-24 is the relative error of one fp32 rounding):
  forward   d_j = fl(x_j - O): 1;  s d: 1;  d - s d: 1;  s + relu: 1.  d_j <= s_j and ds_j/ds_{j-1} = 1 - m d in
            [0, 1], so the levels add: |s_k - ref| <= C_FWD (k + 1) u with C_FWD = 4 (values <= 1).
  backward  along one path from gs_k to Gx_0 that leaves the skeleton chain at level j: 3 u per chain level
            (d, 1 - d, the product), (4 j + 2) u at the branch (s_{j-1} carries 4 j u, 1 - s, the product), and per
            level walked down a 10-term sum (9 u) and a 6-term sum (5 u): 3 (k - j) + 4 j + 2 + 14 (j + 1)
            <= 21 k + 16 <= C_GRAD (k + 1), C_GRAD = 24.
  loss      p = hi or lo of e = expf(-|z|) (1 ulp = 2 u), d = 1 + e (2 u), hi = 1 / d (4 u), lo = e / d (6 u):
            EPS_P = 6; p (1 - p) = hi lo: EPS_HL = 12.  z = fl32(o1 - o0) is part of the definition.  A relative
            error EPS_P u of p moves d_j by at most 2 EPS_P u, which adds C_IN = 12 a level to the gradient's
            count, and moves a sum <g, S(p)> by at most EPS_P u sum |Gx_0| p to first order.
"""
import numpy as np

U = 2.0 ** -24
C_FWD = 4
C_GRAD = 24
C_IN = 12
EPS_P = 6
EPS_HL = 12
SLACK = 1.01  # second-order terms of the (1 + u)^n products

_E_OFF = [(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)]
_D_OFF = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def _windows(x, offs, fill):
    """[len(offs), N, H, W]: x shifted to every window position, `fill` outside the image"""
    N, H, W = x.shape
    pad = np.full((N, H + 2, W + 2), fill, dtype=np.float64)
    pad[:, 1:-1, 1:-1] = x
    return np.stack([pad[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in offs])


def erode(x):
    """-> (E(x), window position of the first minimum)"""
    w = _windows(x, _E_OFF, np.inf)
    sel = np.argmin(w, axis=0)  # the first occurrence
    return np.take_along_axis(w, sel[None], 0)[0], sel


def dilate(x):
    """-> (D(x), window position of the first maximum)"""
    w = _windows(x, _D_OFF, -np.inf)
    sel = np.argmax(w, axis=0)
    return np.take_along_axis(w, sel[None], 0)[0], sel


def _level(xj, sprev):
    e, sel_e = erode(xj)
    o, sel_d = dilate(e)
    u = xj - o
    d = np.maximum(u, 0.0)
    a = d - sprev * d
    return dict(x=xj, e=e, sel_e=sel_e, o=o, sel_d=sel_d, u=u, d=d, a=a, sprev=sprev, s=sprev + np.maximum(a, 0.0))


def skeleton_levels(x, iters):
    """levels 0 .. iters of S(x) for x [N, H, W]; level j holds x_j, E(x_j), O(x_j), both selections, the two relu
    arguments u = x_j - O(x_j) and a = d_j - s_{j-1} d_j, s_{j-1} and s_j"""
    x = np.asarray(x, dtype=np.float64)
    lv = [_level(x, np.zeros_like(x))]
    for _ in range(iters):
        lv.append(_level(lv[-1]["e"], lv[-1]["s"]))
    return lv


def soft_skeleton(x, iters):
    return skeleton_levels(x, iters)[-1]["s"]


def _scatter(g, sel, offs):
    """out[target of q] += g[q], the target of q being q + offs[sel[q]]"""
    N, H, W = g.shape
    n, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    off = np.asarray(offs)
    out = np.zeros_like(g)
    np.add.at(out, (n, y + off[sel, 0], x + off[sel, 1]), g)
    return out


def skeleton_backward(levels, gskel):
    """-> (gx, A): the gradient of sum(gskel * S(x)) by x under the stated rules, and per element the sum of the
    absolute values of the terms that enter it"""
    gs = np.asarray(gskel, dtype=np.float64)
    As = np.abs(gs)
    gxn = np.zeros_like(gs)
    Axn = np.zeros_like(gs)
    for lv in reversed(levels):
        m = lv["a"] > 0
        r = lv["u"] > 0
        on = m & r
        gu = np.where(on, gs * (1.0 - lv["sprev"]), 0.0)
        Au = np.where(on, As * (1.0 + lv["sprev"]), 0.0)
        gs, As = np.where(m, gs * (1.0 - lv["d"]), gs), np.where(m, As * (1.0 + lv["d"]), As)
        ge = gxn - _scatter(gu, lv["sel_d"], _D_OFF)
        Ae = Axn + _scatter(Au, lv["sel_d"], _D_OFF)
        gxn = gu + _scatter(ge, lv["sel_e"], _E_OFF)
        Axn = Au + _scatter(Ae, lv["sel_e"], _E_OFF)
    return gxn, Axn


def fwd_bound(iters):
    return SLACK * C_FWD * (iters + 1) * U


def grad_bound(A, iters):
    return SLACK * C_GRAD * (iters + 1) * U * A


# ---- the conditions under which a comparison is meaningful ----------------------------------------------------
def distinct_inputs(x):
    """every image's values are pairwise distinct: an equality inside a window of some x_j is then the same input
    pixel seen twice, and whichever copy a tie rule picks, the gradient ends at that pixel"""
    return all(np.unique(img).size == img.size for img in np.asarray(x))


def relu_arguments(levels):
    return np.concatenate([np.concatenate([lv["u"].ravel(), lv["a"].ravel()]) for lv in levels])


def selection_margin(levels):
    """the smallest relative gap, over every min and max window of every level, between the extreme and the nearest
    different value of the window (inf if no window holds two values): perturbing the input by less than half of
    it, relatively, changes no selection"""
    best = np.inf
    for lv in levels:
        for src, offs, fill, sign in ((lv["x"], _E_OFF, np.inf, 1.0), (lv["e"], _D_OFF, -np.inf, -1.0)):
            w = sign * _windows(src, offs, fill)  # minima either way
            lo = w.min(axis=0)
            other = np.where(w > lo[None], w, np.inf).min(axis=0)
            ok = np.isfinite(other)
            if ok.any():
                scale = np.maximum(np.abs(other[ok]), np.abs(lo[ok]))
                best = min(best, float(((other[ok] - lo[ok]) / scale).min()))
    return best


# ---- the loss ---------------------------------------------------------------------------------------------------
def logit(out):
    """z of planar fp32 logits [B, nch, H, W]: o1 - o0 rounded to fp32 (nch 2), or o0"""
    out = np.asarray(out, dtype=np.float32)
    return (out[:, 1] - out[:, 0] if out.shape[1] == 2 else out[:, 0]).astype(np.float64)


def cldice(out, tgt, iters=3, smooth=1.0, ignore=None):
    """-> dict: L, gz = dL/dz [B, H, W], and the bounds L_bound and gz_bound (per element, for weight 1) the
    fp32 kernels must keep; p, y, sp = S(p), sy = S(y) and the levels of S(p) for the conditions"""
    z = logit(out)
    tgt = np.asarray(tgt)
    valid = np.ones(tgt.shape, bool) if ignore is None else tgt != ignore
    p = np.where(valid, 1.0 / (1.0 + np.exp(-z)), 0.0)
    y = np.where(valid & (tgt == 1), 1.0, 0.0)
    hl = np.where(valid, p * (1.0 - p), 0.0)
    lp = skeleton_levels(p, iters)
    sp, sy = lp[-1]["s"], soft_skeleton(y, iters)
    a1, a2, b1, b2 = (sp * y).sum(), sp.sum(), (sy * p).sum(), sy.sum()
    tp, ts = (a1 + smooth) / (a2 + smooth), (b1 + smooth) / (b2 + smooth)
    L = 1.0 - 2.0 * tp * ts / (tp + ts)
    dtp, dts = -2.0 * ts * ts / (tp + ts) ** 2, -2.0 * tp * tp / (tp + ts) ** 2
    cA, cB = dtp / (a2 + smooth), dts / (b2 + smooth)
    gx, A = skeleton_backward(lp, cA * (y - tp))
    # A of the top level counts y and tprec as two terms
    _, A = skeleton_backward(lp, np.abs(cA) * (y + tp))
    gz = (gx + cB * sy) * hl
    Agz = (A + np.abs(cB) * sy) * hl
    # errors of the four sums: S(p) to C_FWD (k + 1) u of itself, and the fp32 p under it to EPS_P u of itself
    k1 = iters + 1
    g1, _ = skeleton_backward(lp, np.ones_like(p))
    gy, _ = skeleton_backward(lp, y)
    e_a2 = C_FWD * k1 * U * a2 + EPS_P * U * (np.abs(g1) * p).sum()
    e_a1 = C_FWD * k1 * U * a1 + EPS_P * U * (np.abs(gy) * p).sum()
    e_tp = (e_a1 + tp * e_a2) / (a2 + smooth)
    e_ts = EPS_P * U * b1 / (b2 + smooth)  # S(y) is exact: 0 / 1 maps round nowhere
    L_bound = SLACK * (abs(dtp) * e_tp + abs(dts) * e_ts + 2 * U * abs(L))
    # the factors cA, cB: -2 t^2 / (tp + ts)^2 / (sum + smooth), cast to fp32
    e_c = 4 * (e_tp / tp + e_ts / ts) + e_a2 / (a2 + smooth) + U
    rel = (e_c + e_tp / tp + 3 * U) + (C_GRAD + C_IN) * k1 * U + 2 * U + (EPS_HL + 1) * U + U
    return dict(L=L, gz=gz, L_bound=L_bound, gz_bound=SLACK * rel * Agz, p=p, y=y, sp=sp, sy=sy, levels=lp, tprec=tp,
                tsens=ts)
