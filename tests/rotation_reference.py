"""NumPy restatement of cv2.warpAffine(src, M, (0, 0), INTER_LINEAR, BORDER_CONSTANT 0) as OpenCV 3.4 (imgwarp.cpp) computes it
for float32 images, given the INVERTED matrix (posepaf.rotation.invert_affine).  Test data only: the kernels are checked
against it bit for bit.

    adelta = rint(M0 x 1024), bdelta = rint(M3 x 1024)                 (AB_BITS = 10, cvRound = round half even)
    X0 = rint((M1 y + M2) 1024) + 16, Y0 = rint((M4 y + M5) 1024) + 16   (round_delta = AB_SCALE / INTER_TAB_SIZE / 2)
    X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5                     (INTER_BITS = 5, arithmetic shift)
    sx = X >> 5, fx = X & 31 (the same for y); float32 weights of the 32 x 32 table, exact;
    value = ((v00 w0 + v01 w1) + v10 w2) + v11 w3 in float32; taps outside the source read 0, and a pixel whose 2 x 2 block lies
    wholly outside is exactly 0."""
import numpy as np


def source_coords(m_inv, h, w):
    """fixed-point source coordinates of every destination pixel of an (h, w) output: -> sx, sy, fx, fy int64 (h, w)"""
    M = np.asarray(m_inv, np.float64).reshape(6)
    x = np.arange(w, dtype=np.float64)
    y = np.arange(h, dtype=np.float64)
    adelta = np.rint(M[0] * x * 1024).astype(np.int64)
    bdelta = np.rint(M[3] * x * 1024).astype(np.int64)
    X0 = np.rint((M[1] * y + M[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((M[4] * y + M[5]) * 1024).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    return X >> 5, Y >> 5, X & 31, Y & 31


def warp_affine(src, m_inv):
    """src (H, W) or (H, W, C) float32 -> the same shape, warped with the inverted matrix m_inv (2x3 or 6 doubles)"""
    src = np.asarray(src, np.float32)
    squeeze = src.ndim == 2
    if squeeze:
        src = src[:, :, None]
    H, W, C = src.shape
    sx, sy, fx, fy = source_coords(m_inv, H, W)
    ax = (fx.astype(np.float32) / np.float32(32))
    ay = (fy.astype(np.float32) / np.float32(32))
    one = np.float32(1)
    w0 = (one - ay) * (one - ax)
    w1 = (one - ay) * ax
    w2 = ay * (one - ax)
    w3 = ay * ax

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        return np.where(ok[:, :, None], v, np.float32(0))

    v0, v1, v2, v3 = tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)
    out = v0 * w0[:, :, None]
    out = out + v1 * w1[:, :, None]
    out = out + v2 * w2[:, :, None]
    out = out + v3 * w3[:, :, None]
    outside = (sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0)
    out[outside] = 0
    out = out.astype(np.float32)
    return out[:, :, 0] if squeeze else out
