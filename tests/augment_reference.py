"""NumPy restatement of the training-data transformer's contract (the device stage is pp_augment_batch,
csrc/posepaf_augment.hip).  Test data only: the kernels are checked against it bit for bit.  It follows OpenCV 3.4 (imgwarp.cpp,
resize.cpp, morph.cpp) for 8-bit images, but it is this statement the implementation is held to, not a cv2 run.

    coordinates   rotation_reference.source_coords of the INVERTED matrix at the output size (int64 here, int32 on the device)
    bilinear      a = fx, b = fy: v = (v00 (32-a)(32-b) + v01 a (32-b) + v10 (32-a) b + v11 a b + 512) >> 10, all integer
    border        BORDER_CONSTANT: a tap outside the (h, w) source reads the border value; a block wholly outside gives it
    masks         m = rint_half_even(sum of the 4 x 4 warped values * 0.0625f) (exact in float32), stored float32(m) / float32(255)
    foreground    the minimum over the 3 x 3 neighbours inside the frame
    image         float32(u8) / float32(255)
    joints        x' = (m0 x + m1 y) + m2 in float64, each operation rounded on its own, then rounded to float32; the flag is copied;
                  after a flip the rows of LEFT_PARTS and RIGHT_PARTS are exchanged whole; persons past n_people stay as they were
"""
import numpy as np

from rotation_reference import source_coords

# config/config.py:60 of the reference: nose neck Rsho Relb Rwri Lsho Lelb Lwri Rhip Rkne Rank Lhip Lkne Lank Reye Leye Rear Lear
LEFT_PARTS = [5, 6, 7, 11, 12, 13, 15, 17]      # Lsho Lelb Lwri Lhip Lkne Lank Leye Lear
RIGHT_PARTS = [2, 3, 4, 8, 9, 10, 14, 16]       # Rsho Relb Rwri Rhip Rkne Rank Reye Rear
BORDER = (124, 127, 127)


def warp_u8(src, m_inv, out_h, out_w, border):
    """src uint8 (h, w) or (h, w, C) -> uint8 (out_h, out_w[, C]) warped with the inverted matrix; border: one value per channel"""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    squeeze = src.ndim == 2
    if squeeze:
        src = src[:, :, None]
    H, W, C = src.shape
    bd = np.broadcast_to(np.asarray(border, np.int64).reshape(-1), (C,))
    sx, sy, fx, fy = source_coords(m_inv, out_h, out_w)
    w00, w01, w10, w11 = (32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy

    def tap(yy, xx):
        if H == 0 or W == 0:
            return np.broadcast_to(bd, (out_h, out_w, C))
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        return np.where(ok[:, :, None], v, bd[None, None, :])

    acc = (tap(sy, sx) * w00[:, :, None] + tap(sy, sx + 1) * w01[:, :, None] + tap(sy + 1, sx) * w10[:, :, None]
           + tap(sy + 1, sx + 1) * w11[:, :, None] + 512) >> 10
    outside = (sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0)
    acc = np.where(outside[:, :, None], bd[None, None, :], acc)
    assert acc.min() >= 0 and acc.max() <= 255
    out = acc.astype(np.uint8)
    return out[:, :, 0] if squeeze else out


def area4(plane_u8):
    """uint8 (h, w), h and w multiples of 4 -> uint8 (h / 4, w / 4): rint (half to even) of the 4 x 4 sums * 0.0625f"""
    h, w = plane_u8.shape
    s = plane_u8.astype(np.int64).reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3))
    prod = s.astype(np.float32) * np.float32(0.0625)
    assert np.array_equal(prod.astype(np.float64) * 16, s)        # the product is exact
    return np.rint(prod).astype(np.uint8)


def unit(u8):
    """float32(u8) / float32(255)"""
    return np.asarray(u8).astype(np.float32) / np.float32(255)


def erode3(plane):
    """minimum over the 3 x 3 neighbours inside the frame"""
    h, w = plane.shape
    out = plane.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, ye, xs, xe = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            out[ys:ye, xs:xe] = np.minimum(out[ys:ye, xs:xe], plane[ys + dy:ye + dy, xs + dx:xe + dx])
    return out


def map_joints(m_fwd, joints, n_people, flip):
    """joints float64 (P, 18, 3) -> float32 (P, 18, 3)"""
    m = np.asarray(m_fwd, np.float64).reshape(6)
    j = np.asarray(joints, np.float64)
    out = j.copy()
    n = min(max(int(n_people), 0), j.shape[0])
    x, y = j[:n, :, 0], j[:n, :, 1]
    out[:n, :, 0] = (m[0] * x + m[1] * y) + m[2]
    out[:n, :, 1] = (m[3] * x + m[4] * y) + m[5]
    if flip:
        left, right = out[:n, LEFT_PARTS, :].copy(), out[:n, RIGHT_PARTS, :].copy()
        out[:n, LEFT_PARTS, :] = right
        out[:n, RIGHT_PARTS, :] = left
    return out.astype(np.float32)


def transform(image, mask_miss, mask_all, m_inv, m_fwd, flip, joints, n_people, out_h, out_w, border=BORDER, half=False):
    """One sample: image uint8 (h, w, 3); mask_miss / mask_all uint8 (h, w) or None (constant 255 / 0); joints float64 (P, 18, 3).
    -> image float32 (float16 with half) (out_h, out_w, 3), mask_miss float32 and fg float32 (out_h / 4, out_w / 4), joints float32"""
    h, w = image.shape[:2]
    if mask_miss is None:
        mask_miss = np.full((h, w), 255, np.uint8)
    if mask_all is None:
        mask_all = np.zeros((h, w), np.uint8)
    img = unit(warp_u8(image, m_inv, out_h, out_w, border))
    if half:
        img = img.astype(np.float16)
    miss = unit(area4(warp_u8(mask_miss, m_inv, out_h, out_w, 255)))
    fg = erode3(unit(area4(warp_u8(mask_all, m_inv, out_h, out_w, 0))))
    return img, miss, fg, map_joints(m_fwd, joints, n_people, flip)
