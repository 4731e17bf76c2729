"""Independent numpy restatement of FSR1's two passes (FSR_Pass.glsl with SAMPLE_SLOW_FALLBACK, texture_gather.glsl,
ffx_fsr1.h FsrEasuCon / FsrEasuF / FsrRcasCon / FsrRcasF, ffx_a.h's approximations).

TEST INFRASTRUCTURE.  Written from the GLSL, NOT from include/hk_fsr.h (the per-pixel code the CPU side and the GPU
kernels share), so that tests can pin that header against a second reading of the shaders.  Vectorised over all
output pixels in float32, expressions left to right, nothing fused.  The project's fixed rules for what GLSL leaves
open: `texture()` is post_numpy.linear (clamp-to-edge, the one fixed bilinear evaluation), texelFetch out of bounds
is 0, min / max / clamp are np.fmin / np.fmax (IEEE minNum / maxNum), imageStore rounds to f16 with astype, the bit
tricks work on integer views.  Literal GLSL expressions are folded in Python floats (double) and rounded once.

`mutate` names one deliberate misreading (tests show that each changes some image):
  "gather_order"   fakeTextureGather's returned components rotated by one
  "rcas_clamp"     RCAS's texelFetch taps clamped to the edge instead of 0 outside
  "set_weights"    FsrEasuSetF's four bilinear weights permuted
  "no_dering"      EASU's final min / max clamp dropped
  "no_newton"      APrxMedRcpF1 without its Newton step
"""
from __future__ import annotations

import numpy as np

import post_numpy as pn

F = np.float32
U = np.uint32


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _float(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def prx_lo_rcp(a):
    return _float(U(0x7EF07EBB) - _bits(a))


def prx_med_rcp(a, newton=True):
    b = _float(U(0x7EF19FFF) - _bits(a))
    return b * (-b * a + F(2.0)) if newton else b


def prx_lo_rsq(a):
    return _float(U(0x5F347D74) - (_bits(a) >> U(1)))


def rcp(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        return F(1.0) / a


def min3(x, y, z):
    return np.fmin(x, np.fmin(y, z))


def max3(x, y, z):
    return np.fmax(x, np.fmax(y, z))


def sat(x):
    return np.fmin(np.fmax(x, F(0.0)), F(1.0))


def easu_con(iw, ih, ow, oh):
    """FsrEasuCon with input viewport = input size; con0..con3 as float32 lists."""
    iw, ih, ow, oh = F(iw), F(ih), F(ow), F(oh)
    con0 = [iw * rcp(ow), ih * rcp(oh), F(0.5) * iw * rcp(ow) - F(0.5), F(0.5) * ih * rcp(oh) - F(0.5)]
    con1 = [rcp(iw), rcp(ih), F(1.0) * rcp(iw), F(-1.0) * rcp(ih)]
    con2 = [F(-1.0) * rcp(iw), F(2.0) * rcp(ih), F(1.0) * rcp(iw), F(2.0) * rcp(ih)]
    con3 = [F(0.0) * rcp(iw), F(4.0) * rcp(ih)]
    return con0, con1, con2, con3


def rcas_con(sharpness):
    """FsrRcasCon: exp2(-sharpness), here in float64 rounded to float32."""
    return F(2.0 ** -float(sharpness))


def fake_gather(t, px, py, mutate=None):
    """texture_gather.glsl: (h, w, 4 samples, 4 channels) in the returned order sp4, sp3, sp2, sp1."""
    h, w = t.shape[:2]
    psx, psy = (F(1.0) / F(w)) / F(2.0), (F(1.0) / F(h)) / F(2.0)
    sp3 = pn.linear(t, px + psx, py + psy)
    sp1 = pn.linear(t, px - psx, py - psy)
    psy = psy * F(-1.0)
    sp2 = pn.linear(t, px + psx, py + psy)
    psx, psy = psx * F(-1.0), psy * F(-1.0)
    sp4 = pn.linear(t, px + psx, py + psy)
    order = [sp4, sp3, sp2, sp1]
    if mutate == "gather_order":
        order = order[1:] + order[:1]
    return np.stack(order, axis=-2)


def _set(dir_, len_, w, lA, lB, lC, lD, lE):
    dc, cb = lD - lC, lC - lB
    lenX = np.fmax(np.abs(dc), np.abs(cb))
    lenX = prx_lo_rcp(lenX)
    dirX = lD - lB
    dir_[0] = dir_[0] + dirX * w
    lenX = sat(np.abs(dirX) * lenX)
    lenX = lenX * lenX
    len_ = len_ + lenX * w
    ec, ca = lE - lC, lC - lA
    lenY = np.fmax(np.abs(ec), np.abs(ca))
    lenY = prx_lo_rcp(lenY)
    dirY = lE - lA
    dir_[1] = dir_[1] + dirY * w
    lenY = sat(np.abs(dirY) * lenY)
    lenY = lenY * lenY
    return len_ + lenY * w


def _tap(aC, aW, offx, offy, dir_, len2, lob, clp, c):
    vx = (offx * dir_[0]) + (offy * dir_[1])
    vy = (offx * (-dir_[1])) + (offy * dir_[0])
    vx, vy = vx * len2[0], vy * len2[1]
    d2 = vx * vx + vy * vy
    d2 = np.fmin(d2, clp)
    wB = F(2.0 / 5.0) * d2 + F(-1.0)
    wA = lob * d2 + F(-1.0)
    wB = wB * wB
    wA = wA * wA
    wB = F(25.0 / 16.0) * wB + F(-(25.0 / 16.0 - 1.0))
    w = wB * wA
    return aC + c * w[..., None], aW + w


def easu(image, out_w, out_h, mutate=None):
    """FsrEasuF over every output pixel.  image: (h, w, 4) float32 (the RGBA16F input decoded); returns the stored
    RGBA16F words, (out_h, out_w, 4) uint16."""
    t = np.ascontiguousarray(image, np.float32)
    h, w = t.shape[:2]
    con0, con1, con2, con3 = easu_con(w, h, out_w, out_h)
    iy, ix = np.mgrid[0:out_h, 0:out_w]
    with np.errstate(all="ignore"):
        ppx = ix.astype(np.uint32).astype(np.float32) * con0[0] + con0[2]
        ppy = iy.astype(np.uint32).astype(np.float32) * con0[1] + con0[3]
        fpx, fpy = np.floor(ppx), np.floor(ppy)
        ppx, ppy = ppx - fpx, ppy - fpy
        p0x, p0y = fpx * con1[0] + con1[2], fpy * con1[1] + con1[3]
        p1x, p1y = p0x + con2[0], p0y + con2[1]
        p2x, p2y = p0x + con2[2], p0y + con2[3]
        p3x, p3y = p0x + con3[0], p0y + con3[1]
        bczz = fake_gather(t, p0x, p0y, mutate)
        ijfe = fake_gather(t, p1x, p1y, mutate)
        klhg = fake_gather(t, p2x, p2y, mutate)
        zzon = fake_gather(t, p3x, p3y, mutate)

        def luma(g):  # B * 0.5 + (R * 0.5 + G), per gathered sample
            return g[..., 2] * F(0.5) + (g[..., 0] * F(0.5) + g[..., 1])
        bczzL, ijfeL, klhgL, zzonL = luma(bczz), luma(ijfe), luma(klhg), luma(zzon)
        bL, cL = bczzL[..., 0], bczzL[..., 1]
        iL, jL, fL, eL = (ijfeL[..., k] for k in range(4))
        kL, lL, hL, gL = (klhgL[..., k] for k in range(4))
        oL, nL = zzonL[..., 2], zzonL[..., 3]
        one = F(1.0)
        weights = [(one - ppx) * (one - ppy), ppx * (one - ppy), (one - ppx) * ppy, ppx * ppy]
        if mutate == "set_weights":
            weights = weights[1:] + weights[:1]
        dir_ = [np.zeros_like(ppx), np.zeros_like(ppx)]
        len_ = np.zeros_like(ppx)
        len_ = _set(dir_, len_, weights[0], bL, eL, fL, gL, jL)
        len_ = _set(dir_, len_, weights[1], cL, fL, gL, hL, kL)
        len_ = _set(dir_, len_, weights[2], fL, iL, jL, kL, nL)
        len_ = _set(dir_, len_, weights[3], gL, jL, kL, lL, oL)
        dirR = dir_[0] * dir_[0] + dir_[1] * dir_[1]
        zro = dirR < F(1.0 / 32768.0)
        dirR = prx_lo_rsq(dirR)
        dirR = np.where(zro, one, dirR)
        dir_[0] = np.where(zro, one, dir_[0])
        dir_ = [dir_[0] * dirR, dir_[1] * dirR]
        len_ = len_ * F(0.5)
        len_ = len_ * len_
        stretch = (dir_[0] * dir_[0] + dir_[1] * dir_[1]) * prx_lo_rcp(np.fmax(np.abs(dir_[0]), np.abs(dir_[1])))
        len2 = [one + (stretch - one) * len_, one + F(-0.5) * len_]
        lob = F(0.5) + F((1.0 / 4.0 - 0.04) - 0.5) * len_
        clp = prx_lo_rcp(lob)

        def rgb(g, k):
            return g[..., k, :3]
        f_, g_, j_, k_ = rgb(ijfe, 2), rgb(klhg, 3), rgb(ijfe, 1), rgb(klhg, 0)
        min4 = np.fmin(min3(f_, g_, j_), k_)
        max4 = np.fmax(max3(f_, g_, j_), k_)
        aC = np.zeros(ppx.shape + (3,), np.float32)
        aW = np.zeros_like(ppx)
        taps = [((0.0, -1.0), rgb(bczz, 0)), ((1.0, -1.0), rgb(bczz, 1)), ((-1.0, 1.0), rgb(ijfe, 0)),
                ((0.0, 1.0), rgb(ijfe, 1)), ((0.0, 0.0), rgb(ijfe, 2)), ((-1.0, 0.0), rgb(ijfe, 3)),
                ((1.0, 1.0), rgb(klhg, 0)), ((2.0, 1.0), rgb(klhg, 1)), ((2.0, 0.0), rgb(klhg, 2)),
                ((1.0, 0.0), rgb(klhg, 3)), ((1.0, 2.0), rgb(zzon, 2)), ((0.0, 2.0), rgb(zzon, 3))]
        for (ox, oy), c in taps:
            aC, aW = _tap(aC, aW, F(ox) - ppx, F(oy) - ppy, dir_, len2, lob, clp, c)
        pix = aC * rcp(aW)[..., None]
        if mutate != "no_dering":
            pix = np.fmin(max4, np.fmax(min4, pix))
        out = np.concatenate([pix, np.ones(ppx.shape + (1,), np.float32)], axis=-1)
        return np.ascontiguousarray(out.astype(np.float16)).view(np.uint16)


def _fetch(t, x, y, clamp):
    h, w = t.shape[:2]
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    v = t[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1), :3]
    return v if clamp else np.where(inside[..., None], v, F(0.0))


def rcas(image, sharpness=0.0, con=None, mutate=None):
    """FsrRcasF over every pixel of image, (h, w, 4) float32; con: the RCAS constant (default rcas_con(sharpness)).
    Returns the stored RGBA16F words, (h, w, 4) uint16."""
    t = np.ascontiguousarray(image, np.float32)
    h, w = t.shape[:2]
    con = rcas_con(sharpness) if con is None else F(con)
    y, x = np.mgrid[0:h, 0:w]
    clamp = mutate == "rcas_clamp"
    with np.errstate(all="ignore"):
        b, d = _fetch(t, x, y - 1, clamp), _fetch(t, x - 1, y, clamp)
        e = _fetch(t, x, y, clamp)
        f, hh = _fetch(t, x + 1, y, clamp), _fetch(t, x, y + 1, clamp)
        mn4 = np.fmin(min3(b, d, f), hh)
        mx4 = np.fmax(max3(b, d, f), hh)
        peak_x, peak_y = F(1.0), F(-1.0 * 4.0)
        hit_min = np.fmin(mn4, e) * rcp(F(4.0) * mx4)
        hit_max = (peak_x - np.fmax(mx4, e)) * rcp(F(4.0) * mn4 + peak_y)
        lobe3 = np.fmax(-hit_min, hit_max)
        lobe = np.fmax(F(-(0.25 - (1.0 / 16.0))),
                       np.fmin(max3(lobe3[..., 0], lobe3[..., 1], lobe3[..., 2]), F(0.0))) * con
        rcp_l = prx_med_rcp(F(4.0) * lobe + F(1.0), newton=mutate != "no_newton")
        lobe, rcp_l = lobe[..., None], rcp_l[..., None]
        pix = (lobe * b + lobe * d + lobe * hh + lobe * f + e) * rcp_l
        out = np.concatenate([pix, np.ones((h, w, 1), np.float32)], axis=-1)
        return np.ascontiguousarray(out.astype(np.float16)).view(np.uint16)
