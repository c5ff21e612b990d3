"""Joint lists shared by the scene-renderer tests (CPU and GPU) and by tests/golden/make_golden_scenes.py: the smallest scenes
that reach every branch of the recipe.  All coordinates are float32 values, the type the device renderer reads."""
import numpy as np

SHAPES = ((16, 24), (33, 47), (128, 128))     # (h, w) of the map; the image is 4x that.  33 x 47: w is no multiple of 8
BATCH_MAX_PEOPLE = 12


def _f32(j):
    return np.asarray(j, np.float32)


def random_people(n: int, seed: int, h: int, w: int) -> np.ndarray:
    from posepaf import synth
    return _f32(synth.random_people(n, np.random.default_rng(seed), img_h=4 * h, img_w=4 * w))


def edge_people(h: int, w: int, seed: int = 5) -> np.ndarray:
    """Nine people on a (h, w) map:
    Flags: 0 (annotated, not visible), 1 (annotated, visible) and 2 (absent) all occur -- 0 and 1 are drawn, 2 is not.
    0 a person inside the frame, parts 3 / 7 / 12 flagged 0; 1 the same person again (coincident limbs: count 2 averages); 2 the person moved far left of
    and above the frame (negative window bound: the skip branch); 3 moved right of and below it (empty window); 4 / 5 straddling
    the top-left / bottom-right corner (windows clipped on all four borders between them); 6 joints on .5 cell boundaries
    (x / 4 = 2.5 rounds to 2, 3.5 to 4), nose == neck (a zero-length limb) and a few absent parts; 7 / 8 two more random people."""
    ih, iw = 4 * h, 4 * w
    base = random_people(3, seed, h, w)
    p0 = base[0].copy()
    p0[:, 2] = 1
    p0[[3, 7, 12], 2] = 0                                         # "marked but invisible": annotated, so drawn like flag 1
    centre = p0[:, :2].mean(axis=0)
    p0[:, :2] += np.float32([iw / 2, ih / 2]) - centre           # centred: inside for every shape used here

    def moved(dx, dy):
        q = p0.copy()
        q[:, :2] += np.float32([dx, dy])
        return q
    lo, hi = p0[:, :2].min(axis=0), p0[:, :2].max(axis=0)
    p6 = p0.copy()
    p6[:, 0] = np.float32(10.0) + 4 * np.arange(18, dtype=np.float32)      # x / 4 = 2.5, 3.5, ...: every one a tie
    p6[:, 1] = np.float32(14.0) + 4 * (np.arange(18, dtype=np.float32) % 5)
    p6[0, :2] = p6[1, :2]                                                   # nose on the neck: limb (1, 0) has length zero
    p6[[4, 9, 16], 2] = 2
    p7 = base[1].copy()
    p7[:6, 2] = np.where(p7[:6, 2] < 2, 0, 2)                     # a random person whose head and right arm carry flag 0
    people = [p0, p0.copy(), moved(-(iw + 300), -(ih + 300)), moved(iw + 200, ih + 200),
              moved(-lo[0] - 6, -lo[1] - 6), moved(iw - hi[0] + 6, ih - hi[1] + 6), p6, p7, base[2]]
    return _f32(np.stack(people))


def batch_people(h: int, w: int):
    """people of a batch of four images with 0, 1, 9 and BATCH_MAX_PEOPLE people; every third annotated joint of the last image
    carries flag 0"""
    crowd = random_people(BATCH_MAX_PEOPLE, 32, h, w)
    flat = crowd.reshape(-1, 3)
    annotated = np.flatnonzero(flat[:, 2] < 2)
    flat[annotated[::3], 2] = 0
    return [np.zeros((0, 18, 3), np.float32), random_people(1, 31, h, w), edge_people(h, w), crowd]
