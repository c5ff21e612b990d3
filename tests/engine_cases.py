"""The cases of tests/test_gpu_engine_pipeline.py (the pipelined engine loop against a one-image synchronous run), shared with
tests/test_engine_cases_cpu.py, which pins on the CPU what keeps the GPU test from being vacuous.  No GPU code at import time.

66 images in three padded-shape buckets at B = 16 -> 6 jobs over 5 plans:

    bucket   padded    maps    images   plans
    A        128x128   32x32   37       b = 16, 16, 8
    B        128x192   32x48   21       b = 16, 8
    C         64x128   16x32    8       b = 8        heights 64 / 40 / 17 / 9: on 16-row maps the C++ rules' record depends on
                                                     the image height (on 32-row maps it never does), so a height that lands on
                                                     the wrong image of a batch shows here and nowhere else

The sizes inside a bucket are mixed, so most images leave part of their slot entry unwritten.  Image i shows scene i mod 16 of
its bucket's bank; pixels are seeded random bytes.
"""
import functools

import numpy as np

B = 16
MAX_IMAGE_HW = (128, 192)
INJECT_SCALE = 1e-3
PEOPLE = (1, 2, 3, 4, 2, 3, 1, 5)
N_SCENES = 16
SCENE_SEED0 = 3000
# scenes="device": the joints of image i, the key of its noise, and a noise that makes the scene id matter
DEVICE_MAX_PEOPLE = max(PEOPLE)
DEVICE_NOISE = 0.02
DEVICE_SEED = 4321

SIZES = {
    "A": [(128, 128), (100, 97), (65, 128), (127, 65), (128, 65), (65, 65), (113, 128), (96, 101)],
    "B": [(128, 192), (65, 129), (100, 150), (128, 129), (65, 192), (97, 191), (127, 160)],
    "C": [(64, 128), (40, 65), (17, 100), (9, 128), (17, 97), (9, 65), (17, 127), (9, 66)],
}
COUNTS = {"A": 37, "B": 21, "C": 8}
PADDED = {"A": (128, 128), "B": (128, 192), "C": (64, 128)}
PLANS = {"A": [16, 16, 8], "B": [16, 8], "C": [8]}
N_IMAGES = sum(COUNTS.values())

# what fills every pinned slot before the first job: bytes far from the pad value, so that ONE stale byte in a 4x4 pooling
# cell moves the cell's mean by >= 97 / 255 / 16 = 0.024, i.e. the injected map by 2.4e-5 * weight -- above the 1.5e-5 that one
# binary16 step is worth at the scenes' noise level of 0.02
POISON_LOW, POISON_SPAN = 225, 29


def poison(n: int) -> np.ndarray:
    return ((np.arange(n, dtype=np.int64) * 7) % POISON_SPAN + POISON_LOW).astype(np.uint8)


@functools.lru_cache(None)
def _layout():
    """-> (bucket label of every image, its (h, w)): the buckets shuffled into one another by a fixed permutation"""
    labels = np.array([k for k in "ABC" for _ in range(COUNTS[k])])
    labels = labels[np.random.default_rng(77).permutation(N_IMAGES)]
    seen = {k: 0 for k in "ABC"}
    shapes = []
    for k in labels:
        shapes.append(SIZES[k][seen[k] % len(SIZES[k])])
        seen[k] += 1
    return tuple(labels.tolist()), tuple(shapes)


def bucket(i: int) -> str:
    return _layout()[0][i]


def shapes():
    return list(_layout()[1])


def image(i: int) -> np.ndarray:
    """BGR uint8 (h, w, 3) of image i: seeded random bytes"""
    h, w = _layout()[1][i]
    return np.frombuffer(np.random.default_rng(10_000 + i).bytes(h * w * 3), np.uint8).reshape(h, w, 3)


def scene_index(i: int) -> int:
    return i % N_SCENES


@functools.lru_cache(None)
def bank(label: str) -> np.ndarray:
    """(16, 2, 50, hp / 4, wp / 4) float16: the scene bank of a bucket"""
    from posepaf import synth
    hp, wp = PADDED[label]
    out = np.stack([synth.make_net_output(PEOPLE[s % 8], SCENE_SEED0 + s, hp // 4, wp // 4, dtype=np.float16) for s in range(N_SCENES)])
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def people(i: int) -> np.ndarray:
    """scenes="device": joints (P, 18, 3) of image i's own scene, in the pixels of its padded shape"""
    from posepaf import synth
    hp, wp = PADDED[bucket(i)]
    return synth.random_people(PEOPLE[i % 8], np.random.default_rng(5000 + i), img_h=hp, img_w=wp)


def make_jobs(image_shapes, batch: int = B):
    """The job list evaluate.run_refactored builds: [((hp, wp, b), [image indices])], buckets in order of first appearance, a
    short tail on the smallest plan that takes it."""
    from evaluate import buckets_by_padded_shape, plan_batch
    jobs = []
    for (hp, wp), members in buckets_by_padded_shape(image_shapes).items():
        for b0 in range(0, len(members), batch):
            loc = members[b0:b0 + batch]
            jobs.append(((hp, wp, batch if len(loc) == batch else plan_batch(len(loc), batch)), loc))
    return jobs


def interleave(jobs):
    """round robin over the buckets, each bucket's jobs in their own order: A16 B16 C8 A16 B8 A8 for the set above"""
    queues = {}
    for key, loc in jobs:
        queues.setdefault(key[:2], []).append((key, loc))
    out = []
    while any(queues.values()):
        for q in queues.values():
            if q:
                out.append(q.pop(0))
    return out


def passes():
    """-> (pass 1, pass 2): the interleaved job list and its reverse; run back to back, 12 submits without a synchronisation"""
    first = interleave(make_jobs(shapes()))
    return first, first[::-1]


def single_bucket_jobs(n_jobs: int = 6):
    """b = 16 jobs of bucket A alone (its 37 images, windows of 16): every header such a run can read, stale or not, is a valid
    header of one geometry.  For runs of a deliberately broken engine, which are never part of the suite."""
    members = [i for i in range(N_IMAGES) if bucket(i) == "A"]
    starts = [0, 16, 21, 5, 11, 19, 3, 13]
    return [((128, 128, B), members[s:s + B]) for s in starts[:n_jobs]]


# ------------------------------------------------------------------------------------------------ the stand-in network
def channel_weights() -> np.ndarray:
    return (0.5 + 1.5 * np.random.default_rng(3).random(50)).astype(np.float32)


class TinyModel:
    """NHWC fp16 (n, Hp, Wp, 3) -> (n, 50, Hp / 4, Wp / 4) fp16: channel c = weight[c] * (4x4 mean of colour c mod 3).  The mean
    is fifteen elementwise additions in a fixed order and every other step is elementwise too, so an image's output has the
    same bits at any batch size and in any batch position."""

    def __init__(self, torch, device="cuda"):
        self.weight = torch.from_numpy(channel_weights()).to(device)
        self.colour = (torch.arange(50) % 3).to(device)

    def __call__(self, x):
        n, hp, wp, _ = x.shape
        y = x.float().view(n, hp // 4, 4, wp // 4, 4, 3)
        acc = y[:, :, 0, :, 0]
        for k in range(1, 16):
            acc = acc + y[:, :, k // 4, :, k % 4]
        out = (acc * 0.0625).index_select(3, self.colour) * self.weight
        return out.permute(0, 3, 1, 2).contiguous().half()


def model_numpy(padded_u8: np.ndarray) -> np.ndarray:
    """TinyModel's output (50, hp / 4, wp / 4) float16 for ONE padded image (hp, wp, 3) uint8 as the pre-processing hands it
    over (pixel / 255 rounded to float32, then to float16), step for step in NumPy."""
    hp, wp, _ = padded_u8.shape
    x = (padded_u8.astype(np.float32) / np.float32(255)).astype(np.float16).astype(np.float32)
    y = x.reshape(hp // 4, 4, wp // 4, 4, 3)
    acc = y[:, 0, :, 0]
    for k in range(1, 16):
        acc = acc + y[:, k // 4, :, k % 4]
    out = (acc * np.float32(0.0625))[:, :, np.arange(50) % 3] * channel_weights()
    return np.ascontiguousarray(out.transpose(2, 0, 1)).astype(np.float16)


def padded_image(i: int) -> np.ndarray:
    from posepaf import skeleton as sk
    hp, wp = PADDED[bucket(i)]
    out = np.full((hp, wp, 3), sk.PAD_VALUE, np.uint8)
    im = image(i)
    out[: im.shape[0], : im.shape[1]] = im
    return out


def sensitive_pixel(i: int, maps: np.ndarray):
    """A pixel (y, x, colour) of image i, inside its corner, where ONE grey level must show in `maps` (the image's injected maps
    (2, 50, h4, w4) float16): the stand-in network's own binary16 output is >= 2^-3 there and changes (model_numpy), so by at
    least one step of 2^-13, and the injected value it is scaled into is below 2^-12 in magnitude, where one binary16 step is
    <= 2^-23 < 1e-3 * 2^-13.  -> (y, x, colour, grey level to write)"""
    im = image(i)
    h, w = im.shape[:2]
    base = padded_image(i)
    small = np.abs(maps[0].astype(np.float32)) < 2.0 ** -12
    small[:, h // 4:, :] = False
    small[:, :, w // 4:] = False
    want = model_numpy(base)
    for c, y, x in zip(*np.nonzero(small)):
        if want[c, y, x] < 2.0 ** -3:        # a step of the output is then below 2^-13: not covered by the reasoning above
            continue
        col = int(c) % 3
        old = int(base[4 * y, 4 * x, col])
        new = old + 1 if old < 255 else old - 1
        trial = base.copy()
        trial[4 * y, 4 * x, col] = new
        if model_numpy(trial)[c, y, x] != want[c, y, x]:
            return 4 * int(y), 4 * int(x), col, new
    raise AssertionError("no pixel of this image is provably visible in its maps")
