"""The ragged bucket the original-path tests share (test_original_ragged_cpu.py, test_gpu_original_ragged.py): four images
whose scaled sizes pad to one shape at every scale of [0.5, 1.0, 1.5], with different pads, two half-way roundings
(97 * 0.5 = 48.5 -> 48, 97 * 1.5 = 145.5 -> 146, 86 * 1.5 = 129), two odd sizes, 3 x 4 / 4 x 4 / 4 x 4 / 3 x 4 tiles of
32 x 32, and one image that fills its slot."""
import numpy as np

SCALES = [0.5, 1.0, 1.5]
SIZES = [(120, 100), (128, 128), (97, 115), (86, 127)]
KEY = ((64, 64), (128, 128), (192, 192))          # padded network input per scale; the maps are 16^2, 32^2, 48^2
MAPS = [(16, 16, 0.5), (32, 32, 1.0), (48, 48, 1.5)]
SLOT = (128, 128)
# (people, seed) per image, picked on the CPU (test_original_ragged_cpu.py): every image shows at least one person the
# oracle assembles, and no part has more than 64 peaks
SCENES = [(2, 7101), (3, 7102), (2, 7103), (2, 7104)]
EQUAL_SCENES = [(2, 7201), (3, 7202), (2, 7203), (3, 7204)]     # the all-(128, 128) bucket
CORNER_IMAGE = 2                                  # this image also gets a peak on its own last row and last column
CFG = {"offset_radius": 3, "thre2": 0.05, "mid_num": 40}


def pads(size):
    """[(pad_down, pad_right)] per scale of an image: padded shape minus cv2.resize's round-half-to-even size"""
    h, w = size
    return [(ph - int(round(h * s)), pw - int(round(w * s))) for s, (ph, pw) in zip(SCALES, KEY)]


def scene_maps(size, people, seed, dtype=np.float16):
    """network outputs (2, 50, h, w) of one image at the three scales: the same people, inside the image"""
    from posepaf import synth
    return synth.make_scene_at_scales(people, seed, MAPS, dtype=dtype, img=min(size))[0]


def add_corner_peak(heat, size):
    """a nose peak on the image's last row and last column (heat: (20, H, W) float64, numpy or torch, in place)"""
    h, w = size
    heat[0, h - 1, w - 1] = 0.9
    heat[0, h - 2, w - 2] = 0.5


def oracle_image(oracle, size, people, seed, corner=False, dtype=np.float16):
    """the oracle's accumulators, peaks and persons of one image run alone"""
    h, w = size
    heat, paf = np.zeros((20, h, w)), np.zeros((30, h, w))
    for o, (pd, pr) in zip(scene_maps(size, people, seed, dtype), pads(size)):
        oracle.predict_accumulate(o, pd, pr, h, w, len(SCALES), heat, paf)
    if corner:
        add_corner_peak(heat, size)
    rows = oracle.find_peaks_original(heat, 0.1)
    persons, _ = oracle.py_find_humans_f64(rows, paf, h)
    return heat, paf, rows, persons
