#!/usr/bin/env python3
"""evaluate.py -- the reference's evaluation loop (evaluate.py:235-330) on the MI355X-native path.

    python evaluate.py --run_refactor --run_cpp --synthetic 5000 [--batch 128] [--dump_name results.json]
    python evaluate.py --run_refactor --run_cpp -p weights.pth --ann_file person_keypoints_val2017.json --img_dir val2017
    python evaluate.py --gpus 8 --run_refactor --run_cpp --synthetic 5000          # launches its own 8 ranks
    python evaluate.py --synthetic 512 --batch 32 --scales 1.0 --test_cfg thre2=0.05 mid_num=40 remove_recon=1   # original
        path with the reference's test_cfg keys as run-time values (or --config_file PATH: the [param] section of an INI file)
    python evaluate.py --run_refactor --run_cpp --synthetic 256 --render_dir out/    # + every image with its skeletons drawn
    python evaluate.py --synthetic 64 --batch 32 --scales 0.5 1.0 1.5 --render_limbs_dir out/   # original path: + every image with
        its people in the demo's ellipse / alpha-blend style, drawn on the GPU from the device-side records
    python evaluate.py --run_refactor --run_cpp --synthetic 5000 --ap device         # rows + OKS matching on every rank's own GPU,
        AP / AP50 / AP75 / AP(M) / AP(L) / AR ... (--ap host: the same twelve values from the host function, for comparison)
    python evaluate.py --synthetic 256 --batch 32 --scales 0.5 1.0 1.5 --sizes 512x480,480x512,500x475   # original path: sizes
        that pad alike at every scale share one ragged bucket (POSEPAF_ORIGINAL_BUCKETS=exact: group by exact size instead)
    python evaluate.py --run_refactor --run_cpp --synthetic 5000 --scenes device     # 5000 distinct scenes, each rendered on the
        GPU from its joint list inside the batch's graph (default --scenes bank: 64 host-rendered scenes, image i shows i mod 64)
    python evaluate.py --val_loss --synthetic 512 --batch 32                         # the reference's validation loss (multi-scale
        focal L2 over 4 stacks x 5 scales, models/loss_model.py) of the fused model against device-rendered targets, per stack / scale
    python evaluate.py --val_loss --ann_file F --img_dir D --mask_miss segm          # the same, masked by the reference's mask_miss,
        rasterised on the GPU from the annotations' polygons and crowd run-length code (pp_coco_masks_u8)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 evaluate.py --synthetic 5000 ...

What is kept from the reference: the flags --run_refactor / --run_cpp (:53-54; --run_cpp selects the C++ pafprocess rules --
the README's 65.8-AP / 7.3-fps row -- and its absence the pure-Python rules), the COCO annotation input with the
person-image filter (:237-254), the per-image result format (append_result :182-209), the COCO-style JSON dump (:269-270)
and the keypoint AP against the annotation's ground truth (:274-279, here posepaf/oks_eval.py because pycocotools is absent).

What changes: the refactored path runs on posepaf.engine.InferenceEngine -- THE SAME engine bench.py times: images are
decoded by background threads straight into pinned slots, uploaded on a copy stream under the previous batch's compute,
padded / normalised / mirrored by pp_preprocess_u8_ragged, and forward + post-processing replay from one HIP graph per
bucket.  Images are sharded i mod W over the ranks; the only exchange is one RCCL all-gather of the fixed-size records.
Reported speed = all images / MAX-over-ranks wall time of the loop (loading, upload, compute, record gather included).

Image sizes differ (COCO val2017 does): the reference pads every image to a multiple of 64 (utils/parse_skeletons.py:54,
utils/util.py:44-65) and runs it alone; here a rank's images are BUCKETED by padded shape and each bucket runs in batches;
the per-image `img_h` of process_paf (evaluate.py:110) travels with the batch as a device array.

Data sources:
  --ann_file F --img_dir D   COCO keypoint annotation JSON (read with `json`) + image directory (decoded with PIL, RGB -> BGR
                             like cv2.imread; libjpeg builds may differ in the last bit: unpinned)
  --images DIR               a directory of image files or .npy BGR uint8 arrays, no ground truth
  --synthetic N              random uint8 images; ground-truth-style pose scenes are injected into the network output (a
                             randomly initialised network emits no peaks) and serve as ground truth for the OKS evaluation
"""
import argparse
import glob
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from posepaf import coco, dist as pdist, oks_eval, skeleton as sk, synth  # noqa: E402
from posepaf._lib import RECORD_BYTES  # noqa: E402
from posepaf.engine import padded_shape  # noqa: E402

IMAGE_EXT = (".jpg", ".jpeg", ".png", ".bmp")
SCENE_BANK = 64          # --scenes bank: distinct synthetic scenes per bucket shape (image i shows scene i mod 64)
SCENE_SEED = 20_000      # --scenes device: key of the counter-based noise (the scene id is the image's index in the set)


def parse(argv=None):
    ap = argparse.ArgumentParser(description="PoseNet evaluation (MI355X-native path)")
    ap.add_argument("--run_refactor", action="store_true")
    ap.add_argument("--run_cpp", action="store_true")
    ap.add_argument("--checkpoint_path", "-p", default=None, help="reference checkpoint (.pth with a 'weights' entry)")
    ap.add_argument("--arch", choices=("posenet", "final", "auto"), default="posenet",
                    help="network architecture: posenet = models/posenet.py (the development variant, default), final = models/posenet_final.py "
                         "(the published 3- / 4-stage IMHN), auto = decided from the checkpoint's keys")
    ap.add_argument("--ann_file", default=None, help="COCO keypoint annotation JSON (evaluate.py:237-246)")
    ap.add_argument("--img_dir", default=None, help="directory of the annotation's images (evaluate.py:263)")
    ap.add_argument("--all_images", action="store_true", help="with --ann_file: every image, not only those with a person "
                                                              "annotation (the reference's NUM_TEST_IMG > 0 branch, :247-248)")
    ap.add_argument("--inject_gt", action="store_true", help="with --ann_file and no trained weights: add GT-style maps rendered "
                                                             "from the annotation's keypoints to the network output")
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic images")
    ap.add_argument("--sizes", default="512x512", help="synthetic image sizes HxW[,HxW...], cycled over the image index")
    ap.add_argument("--images", default=None, help="directory of image files / .npy BGR uint8 arrays (any sizes)")
    ap.add_argument("--limit", type=int, default=0, help="evaluate only the first N images of the set")
    ap.add_argument("--gpus", type=int, default=1, help="> 1 without WORLD_SIZE: launch that many ranks (one per GPU)")
    ap.add_argument("--batch", type=int, default=128, help="images per GPU per step")
    ap.add_argument("--workers", type=int, default=0, help="decode threads per rank (0 = CPU share of this rank, <= 16)")
    ap.add_argument("--no_graph", action="store_true", help="launch eagerly instead of replaying HIP graphs")
    ap.add_argument("--dump_name", default="results.json")
    ap.add_argument("--people", type=int, nargs="*", default=[1, 2, 3, 4, 6, 8, 10, 5])
    ap.add_argument("--scales", type=float, nargs="*", default=None,
                    help="without --run_refactor: predict's `multiplier` list (the reference hard-codes [1.0], "
                         "utils/parse_skeletons.py:188); e.g. 0.5 1.0 1.5 for BASELINE config 5")
    ap.add_argument("--rotation_search", type=float, nargs="+", default=None, metavar="A",
                    help="without --run_refactor: test-time rotation angles in degrees (the INI's rotation_search, "
                         "utils/config_reader.py:23); every (scale, angle) entry is run and averaged.  Default 0 (no rotation). "
                         "--run_refactor refuses a non-zero angle: the reference's refactored path keeps only the last angle's "
                         "maps, rotated about a misplaced centre, and the batched graph engine does not implement that")
    ap.add_argument("--test_cfg", nargs="+", default=None, metavar="KEY=VALUE",
                    help="without --run_refactor: run-time values of the reference's test_cfg (utils/config [param]) read by "
                         "find_peaks / find_connections / find_humans: thre1 thre2 connect_ration mid_num len_rate connection_tole "
                         "offset_radius remove_recon, e.g. --test_cfg thre2=0.05 mid_num=40 remove_recon=1.  The C++ pafprocess "
                         "rules (--run_cpp) have these compiled in, as in the reference, and refuse the option")
    ap.add_argument("--config_file", default=None, metavar="PATH",
                    help="without --run_refactor: take those values from the [param] section of a file in the reference's INI "
                         "layout (utils/config); --test_cfg entries override it")
    ap.add_argument("--render_dir", default=None, metavar="DIR",
                    help="with --run_refactor: draw every image's skeletons on the GPU (pp_draw_humans_u8, the refactored branch "
                         "of demo_image.py:174-192, inside the batch's graph) and write each image's own (h, w) canvas to "
                         "DIR/<index in the set>.npy (BGR uint8).  The original path refuses the option: its ellipse drawing is "
                         "--render_limbs_dir")
    ap.add_argument("--render_limbs_dir", default=None, metavar="DIR",
                    help="without --run_refactor: draw every image's people on the GPU in the style of the demo's original branch "
                         "(pp_draw_limbs_u8: demo_image.py:218-240, rotated ellipses and joint rings blended 0.4 / 0.6) from the "
                         "batch's device-side records, and write each image's own (h, w) canvas to DIR/<index in the set>.npy "
                         "(BGR uint8).  --run_refactor refuses the option: that path's style is --render_dir")
    ap.add_argument("--render_format", choices=("npy", "png"), default="npy",
                    help="file format of --render_dir / --render_limbs_dir: .npy always works, .png goes through PIL (as "
                         "demo_image.save_image)")
    ap.add_argument("--ap", choices=("host", "device"), default=None,
                    help="report the keypoint AP with the area-range columns (AP, AP50, AP75, APm, APl, AR, AR50, AR75, ARm, ARl; "
                         "oks_eval.evaluate_keypoints_ranges) and the seconds of the evaluation's steps.  device: every rank builds "
                         "the result rows and matches them against its shard's ground truth on its own GPU (pp_coco_rows_f32, "
                         "pp_oks_match), rank 0 accumulates; host: rank 0 does all of it in Python.  Without the option the report "
                         "is evaluate_keypoints' (range `all` only), as before")
    ap.add_argument("--val_loss", action="store_true",
                    help="a mode of its own: the reference's validation loss (MultiTaskLoss.focal_l2_loss over every stack and scale, "
                         "models/loss_model.py:23-81, :133-161; train*.py test()) of the fused model, computed on the device "
                         "(pp_focal_l2_terms).  Per batch: pad / normalise as the refactored path does, model(x, all_preds=True), the "
                         "targets rendered on the device from the image's own joints (--synthetic: its people; --ann_file: its "
                         "annotations) with reverse_kp and no noise, mask of ones unless --mask_miss segm.  Takes "
                         "--batch, --sizes, --arch, -p; prints one JSON line.  Refuses --scales, --rotation_search, --test_cfg, "
                         "--config_file, --render_dir, --render_limbs_dir, --ap and --scenes bank")
    ap.add_argument("--mask_miss", choices=("ones", "segm"), default="ones",
                    help="with --val_loss --ann_file: segm masks the loss with the reference's mask_miss, rasterised on the device from "
                         "the annotations' polygons and crowd run-length code (pp_coco_masks_u8, INTEGRATION section 19) and brought "
                         "to stride 4 by the data transformer's 4 x 4 area rule under the identity matrix (section 17); an image with "
                         "more than one crowd annotation is skipped and counted.  ones (default): no mask")
    ap.add_argument("--scenes", choices=("bank", "device"), default=None,
                    help="where the injected scenes (--synthetic, --inject_gt) come from.  bank: rendered on the host before the "
                         "run and kept in HBM -- 64 per bucket shape for --synthetic (image i shows scene i mod 64), one per image "
                         "for --inject_gt.  device (with --run_refactor): every image's own scene, rendered from its joint list "
                         "inside the batch's graph (pp_render_scenes) -- --synthetic N shows N distinct scenes and --inject_gt "
                         "needs neither the bank nor --limit")
    ap.add_argument("--scene_noise", type=float, default=0.02,
                    help="--synthetic: sigma of the noise added to the injected scenes (both --scenes modes; the device renderer "
                         "draws it from a counter-based generator, so the two modes' noise values differ)")
    a = ap.parse_args(argv)
    a.scenes_given, a.scenes = a.scenes, a.scenes or "bank"
    if a.scene_noise < 0:
        ap.error("--scene_noise must be >= 0")
    a.test_cfg_dict = None
    if a.test_cfg is not None or a.config_file is not None:
        try:
            cfg = sk.read_config_file(a.config_file) if a.config_file else {}
            cfg.update(sk.parse_test_cfg_items(a.test_cfg))
            a.test_cfg_dict = sk.merge_test_cfg(cfg)
        except (ValueError, OSError) as e:
            ap.error(str(e))
    return a


def buckets_by_padded_shape(shapes):
    """indices grouped by padded (Hp, Wp), each group in ascending index order; groups ordered by first appearance"""
    out = {}
    for k, (h, w) in enumerate(shapes):
        out.setdefault(padded_shape(h, w), []).append(k)
    return out


def plan_batch(n_left: int, B: int) -> int:
    """batch of the plan that takes `n_left` (< B) trailing images of a bucket: B, B/2, B/4 ... >= 8, the smallest that fits"""
    b = B
    while b // 2 >= max(n_left, 8):
        b //= 2
    return b


def read_bgr(path: str) -> np.ndarray:
    """cv2.imread(path) (evaluate.py:72): BGR uint8 (H, W, 3)"""
    if path.endswith(".npy"):
        return np.load(path)
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))[:, :, ::-1]


# ------------------------------------------------------------------------------------------------ data sources
class CocoSource:
    """The annotation file of evaluate.py:237-254 read with `json`: image list (person images only unless all_images),
    file names, sizes, and the ground truth COCOeval would use."""

    def __init__(self, ann_file, img_dir, all_images=False, limit=0, inject_gt=False):
        doc = json.load(open(ann_file))
        images = {im["id"]: im for im in doc["images"]}
        person = [c["id"] for c in doc.get("categories", []) if c.get("name") == "person"] or [1]
        anns = [a for a in doc.get("annotations", []) if a.get("category_id") in person]
        with_person = sorted({a["image_id"] for a in anns})          # getImgIds(catIds=person), :252-254
        ids = sorted(images) if all_images else with_person
        if limit:
            ids = ids[:limit]
        self.image_ids = ids
        self.files = [os.path.join(img_dir, images[i]["file_name"]) for i in ids]
        self._shapes = [(int(images[i]["height"]), int(images[i]["width"])) for i in ids]
        keep = set(ids)
        self.gts = {i: [] for i in ids}
        self.segm = {i: [] for i in ids}         # every person annotation in annotation order, for --mask_miss segm
        for a in anns:
            if a["image_id"] in keep:
                self.segm[a["image_id"]].append({"segmentation": a.get("segmentation"), "iscrowd": int(a.get("iscrowd", 0)),
                                                 "num_keypoints": int(a.get("num_keypoints", 0))})
        for a in anns:
            if a["image_id"] in keep and "keypoints" in a:
                self.gts[a["image_id"]].append({"keypoints": a["keypoints"], "area": float(a["area"]), "bbox": a.get("bbox"),
                                                "num_keypoints": int(a.get("num_keypoints", 0)),
                                                "iscrowd": int(a.get("iscrowd", 0))})
        self.has_scenes = bool(inject_gt)

    def __len__(self):
        return len(self.image_ids)

    def shape(self, i):
        return self._shapes[i]

    def load(self, i):
        im = read_bgr(self.files[i])
        if im.shape[:2] != self._shapes[i]:
            raise SystemExit(f"{self.files[i]}: decoded size {im.shape[:2]} != annotation {self._shapes[i]}")
        return im

    scene_noise = 0.0        # the injected annotation scenes carry no noise, in either --scenes mode

    def scene_joints(self, i, hp=None, wp=None):
        """joints (P, 18, 3) of image i's injected scene: the annotation's own keypoints (COCO order -> the 18 CMU parts, neck =
        shoulder midpoint as in the reference's data pipeline; posepaf.synth_device.coco_to_joints)"""
        from posepaf.synth_device import coco_to_joints
        return coco_to_joints(self.gts[self.image_ids[i]])

    def max_people(self, indices):
        return max([len(self.gts[self.image_ids[i]]) for i in indices] + [1])

    def distinct_scenes(self, device):
        return len(self.image_ids)

    def bank_for_bucket(self, hp, wp, indices):
        """--inject_gt --scenes bank (no weights offline): one GT-style scene per image, rendered on the host from the
        annotation's own keypoints and kept in HBM."""
        if len(indices) * 2 * 50 * (hp // 4) * (wp // 4) * 2 > 64 << 30:
            raise SystemExit("--inject_gt --scenes bank keeps one scene per image in HBM: use --limit, or --scenes device")
        scenes = []
        for i in indices:
            base = synth.render_maps(self.scene_joints(i), hp // 4, wp // 4)
            scenes.append(np.stack([base, synth.mirror_sample(base)]).astype(np.float16))
        return np.stack(scenes), {int(i): k for k, i in enumerate(indices)}


class DirSource:
    def __init__(self, d, limit=0):
        files = sorted(f for f in glob.glob(os.path.join(d, "*")) if f.lower().endswith(IMAGE_EXT + (".npy",)))
        self.files = files[:limit] if limit else files
        self.image_ids = [os.path.splitext(os.path.basename(f))[0] for f in self.files]
        self.gts, self.has_scenes = {}, False
        self._shapes = {}

    def __len__(self):
        return len(self.files)

    def shape(self, i):
        if i not in self._shapes:
            f = self.files[i]
            if f.endswith(".npy"):
                self._shapes[i] = tuple(np.load(f, mmap_mode="r").shape[:2])
            else:
                from PIL import Image
                with Image.open(f) as im:       # header only
                    self._shapes[i] = (im.height, im.width)
        return self._shapes[i]

    def load(self, i):
        return read_bgr(self.files[i])


class SyntheticSource:
    """Random uint8 images; image i shows scene (i mod 64) of its bucket shape with people[i mod len(people)] persons -- or,
    with per_image (--scenes device), its OWN scene: seed 20_000 + i, people[i mod len(people)] persons."""

    def __init__(self, n, sizes, people, noise=0.02, per_image=False):
        self.n, self.sizes, self.people = n, sizes, people
        self.scene_noise, self.per_image = float(noise), bool(per_image)
        self.image_ids = list(range(n))
        self.gts, self.has_scenes = {}, True
        self._scenes, self._joints = {}, {}

    def __len__(self):
        return self.n

    def shape(self, i):
        return self.sizes[i % len(self.sizes)]

    def load(self, i):
        h, w = self.shape(i)
        rng = np.random.default_rng(10_000 + i)
        return np.frombuffer(rng.bytes(h * w * 3), np.uint8).reshape(h, w, 3)

    def scene_slot(self, i):
        return i if self.per_image else i % SCENE_BANK

    def joints(self, slot, hp, wp):
        """ground-truth joints (P, 18, 3) of scene `slot` at padded shape (hp, wp): the people scene() renders, without
        rendering them (synth.make_scene draws them first from the same generator)"""
        key = (slot, hp, wp)
        if key not in self._joints:
            self._joints[key] = synth.random_people(self.n_people(slot), np.random.default_rng(20_000 + slot), img_h=hp, img_w=wp)
        return self._joints[key]

    def scene_joints(self, i, hp, wp):
        return self.joints(self.scene_slot(i), hp, wp)

    def max_people(self, indices):
        return max(list(self.people) + [1])

    def distinct_scenes(self, device):
        return self.n if device else len({(self.scene_slot(i), padded_shape(*self.shape(i))) for i in range(self.n)})

    def bank_for_bucket(self, hp, wp, indices):
        return np.stack([self.scene(s, hp, wp)[0] for s in range(SCENE_BANK)]), {int(i): self.scene_slot(int(i)) for i in indices}

    def n_people(self, slot):
        return self.people[slot % len(self.people)]

    def scene(self, slot, hp, wp):
        """(network-output-shaped scene, ground-truth joints) of bank slot `slot` at padded shape (hp, wp)"""
        key = (slot, hp, wp)
        if key not in self._scenes:
            self._scenes[key] = synth.make_scene(self.n_people(slot), 20_000 + slot, h=hp // 4, w=wp // 4, noise=self.scene_noise,
                                                 dtype=np.float16)
        return self._scenes[key]


# ------------------------------------------------------------------------------------------------ the two loops
def run_refactored(a, src, mine, model, post, dev, rank, world):
    """Refactored path on the shared engine.  -> (device uint8 records of this rank's images in local order, seconds)"""
    from posepaf import fused_model
    from posepaf.engine import InferenceEngine, run_jobs
    B = a.batch
    shapes = [src.shape(int(i)) for i in mine]
    groups = buckets_by_padded_shape(shapes)
    max_hw = (max([padded_shape(*s)[0] for s in shapes] + [64]), max([padded_shape(*s)[1] for s in shapes] + [64]))
    device_scenes = src.has_scenes and a.scenes == "device"
    scene_kw = {}
    if device_scenes:   # every image's scene is rendered from its joint list inside the batch's graph: no bank
        from posepaf import synth_device
        most = src.max_people([int(i) for i in mine])
        if most > synth_device.MAX_PEOPLE:
            raise SystemExit(f"--scenes device renders at most {synth_device.MAX_PEOPLE} people per image, an image here has {most}: "
                             "use --scenes bank")
        scene_kw = dict(scenes="device", max_people=most, scene_noise=src.scene_noise, scene_seed=SCENE_SEED)
    eng = InferenceEngine(model, post, B, dev.index, rules="cpp" if a.run_cpp else "py", use_graph=not a.no_graph,
                          inject_scale=1e-3 if src.has_scenes else None, max_image_hw=max_hw, render=bool(a.render_dir),
                          progress=(lambda m: print(f"[evaluate] {m}", file=sys.stderr, flush=True)) if rank == 0 else None,
                          **scene_kw)
    jobs = []
    for (hp, wp), members in groups.items():
        for b0 in range(0, len(members), B):
            loc = members[b0:b0 + B]
            jobs.append((eng.plan(hp, wp, B if len(loc) == B else plan_batch(len(loc), B)), loc))
    # untimed set-up: scene banks, kernel choice per layer shape (rank 0 tunes, the others take its table), graph capture
    bank_slot = {}
    if src.has_scenes and not device_scenes:
        banks = {}
        for (hp, wp), members in groups.items():
            arr, where = src.bank_for_bucket(hp, wp, [int(mine[k]) for k in members])
            banks[(hp, wp)] = torch.from_numpy(arr).to(dev)
            bank_slot.update(where)
        for p in eng.plans.values():
            eng.set_bank(p, banks[(p.hp, p.wp)])
    fused_model.load_table()
    if world > 1:
        import torch.distributed as dist
        if rank == 0:
            for p in eng.plans.values():
                eng.prepare(p)
        box = [fused_model.table_entries() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        fused_model.install_entries(box[0])
    for p in eng.plans.values():
        eng.prepare(p)
    if rank == 0:
        fused_model.save_table()
    local = torch.zeros((max(len(mine), 1), RECORD_BYTES), dtype=torch.uint8, device=dev)

    def fill(k_local, j, sizes, idx, imgs, n_people=None, joints=None):
        i = int(mine[k_local])
        im = src.load(i)
        h, w = im.shape[:2]
        imgs[j, :h, :w] = im
        sizes[0, j], sizes[1, j] = h, w
        if device_scenes:   # the image's own people travel with it; its index in the set keys the noise
            pj = src.scene_joints(i, *padded_shape(h, w))
            p = pj.shape[0]
            joints[j, :p] = pj
            joints[j, p:, :, 2] = 2
            n_people[j] = p
            idx[j] = i
        elif src.has_scenes:
            idx[j] = bank_slot[i]

    workers = a.workers or max(1, min(16, (len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8) // max(1, min(world, 8))))
    n_rendered = 0
    if a.render_dir:
        from demo_image import save_image
        os.makedirs(a.render_dir, exist_ok=True)
    eng.sync()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    t0 = time.perf_counter()

    def save_canvases(plan, loc):   # the canvas is the plan's until its next submit: bring it to the host now (waits for this batch)
        nonlocal n_rendered
        canvases = plan.canvas[: len(loc)].cpu().numpy()
        for j, k_local in enumerate(loc):
            h, w = shapes[k_local]
            save_image(os.path.join(a.render_dir, "%06d.%s" % (int(mine[k_local]), a.render_format)), canvases[j, :h, :w])
            n_rendered += 1

    run_jobs(eng, jobs, fill, local, workers, depth=2, on_batch=save_canvases if a.render_dir else None)
    eng.sync()
    dt = time.perf_counter() - t0
    info = {"plans": sorted(eng.plans), "decode_threads": workers,
            "conv_table": fused_model.table_hash(), "launch": "eager" if a.no_graph else "hipGraph replay"}
    if a.render_dir:
        info["rendered_files"] = n_rendered
    if src.has_scenes:
        info["scenes"] = "device" if device_scenes else "bank"
        info["distinct_scenes"] = src.distinct_scenes(device_scenes)
    if a.run_cpp:   # where pp_process_batch kept the maps it was handed (dtype and shape of each bucket's network output)
        kinds = {post.map_residency(p.maps.dtype, p.maps.shape[3], p.maps.shape[4]) for p in eng.plans.values() if p.maps is not None}
        if kinds:
            info["map_residency"] = kinds.pop() if len(kinds) == 1 else "mixed"
    return local.view(-1), dt, info


def run_original(a, src, mine, model, post, dev):
    """evaluate.py:81-89 without --run_refactor: predict + find_peaks + find_connections + find_humans at image resolution,
    with a real scale search.  Images are grouped by posepaf.original_path.bucket_key: those whose scaled sizes pad to one shape
    at EVERY scale share the forwards.  A group of one size runs the equal-size kernels; a mixed group is a ragged bucket: the
    images sit in the corners of equal slots, every image is resized / padded / cropped / searched at its own size
    (pp_resize_u8_cubic_ragged, pp_preprocess_u8_ragged, pp_original_accumulate_all_ragged, pp_original_finish_ragged) and
    comes out bit for bit as it does alone.  POSEPAF_ORIGINAL_BUCKETS=exact groups by exact size instead (A/B runs), and so
    does a --rotation_search with a non-zero angle (the warped accumulation has no ragged form).  Per batch the images are
    decoded by a thread pool into a pinned buffer (uploaded while the previous batch computes), every scale runs
    resize -> pad / normalise / mirror -> forward, and ALL scales are accumulated by one launch (pp_original_accumulate_all).
    With --rotation_search every (scale, angle) entry is one more forward: the padded input is rotated by the pre-processing
    kernel and the entry's x4 maps are warped back inside the same launch (pp_original_accumulate_all_affine).
    Synthetic runs take their scenes from a device-resident bank per (size, scale, angle) (64 scenes), like the refactored
    path; a rotated entry's scenes are rendered at the rotated positions (synth.make_scene_at_scales).  The banks of a ragged
    bucket's sizes have equal map shapes and are concatenated once per bucket.
    With --render_limbs_dir every batch is drawn after its finish from the records where they are (pp_draw_limbs_u8, a ragged
    bucket with its own size rows) onto a canvas of the group's own -- the staged images are overwritten two batches later --
    and each image's corner is written out."""
    from concurrent.futures import ThreadPoolExecutor
    from posepaf.original_path import (OriginalPathProcessor, RaggedBucket, RaggedUnsupported, group_by_bucket_key,
                                       preprocess_ragged, resize_images_u8)
    from posepaf.pipeline import preprocess_batch
    from posepaf.rotation import input_and_map_inverses
    B, scales = a.batch, a.scales or [1.0]
    angles = [float(v) for v in (a.rotation_search or [0.0])]
    n_div = len(scales) * len(angles)
    thre1 = 0.1
    if a.test_cfg_dict is not None:
        post.set_test_cfg(a.test_cfg_dict)
        thre1 = a.test_cfg_dict["thre1"]
    shapes = [src.shape(int(i)) for i in mine]
    exact = os.environ.get("POSEPAF_ORIGINAL_BUCKETS", "") == "exact" or any(ang != 0.0 for ang in angles)
    groups = group_by_bucket_key(shapes, scales, exact)
    local = torch.zeros((max(len(mine), 1), RECORD_BYTES), dtype=torch.uint8, device=dev)
    scale = torch.tensor(1e-3, dtype=torch.float16, device=dev)
    workers = a.workers or max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8))
    pool = ThreadPoolExecutor(max_workers=workers)
    banks = {}

    def scene_bank(H, W, fh, fw, sc, ang):
        entry = (fh, fw, float(sc)) if ang == 0.0 else (fh, fw, float(sc), ang)
        return np.stack([synth.make_scene_at_scales(src.n_people(s_), 20_000 + s_, [entry], noise=getattr(src, "scene_noise", 0.02),
                                                    img=H)[0][0]
                         for s_ in range(SCENE_BANK)])

    def setup_exact(H, W):   # convolution shapes of every scale, scene banks of one image size
        if (H, W) in banks:
            return
        banks[(H, W)] = True
        warm = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=dev)
        for sc in scales:
            x = preprocess_batch(resize_images_u8(warm, float(sc)), True, torch.float16)
            model(x)
            if src.has_scenes:
                fh, fw = x.shape[1] // 4, x.shape[2] // 4
                for ang in angles:
                    banks[(H, W, float(sc), ang)] = torch.from_numpy(scene_bank(H, W, fh, fw, sc, ang)).to(dev)

    def setup_ragged(key, members):   # one warm-up forward per scale for the whole bucket; its sizes' banks, concatenated
        sizes = sorted({shapes[k] for k in members})
        for sc, (ph, pw) in zip(scales, key):
            model(torch.zeros((2 * B, ph, pw, 3), dtype=torch.float16, device=dev))
            if src.has_scenes:
                banks[(key, float(sc))] = torch.from_numpy(np.concatenate(
                    [scene_bank(H, W, ph // 4, pw // 4, sc, 0.0) for (H, W) in sizes])).to(dev)
        banks[(key, "sizes")] = {hw: n for n, hw in enumerate(sizes)}

    with torch.no_grad():   # untimed set-up per group
        for key, members, ragged in groups:
            if ragged:
                setup_ragged(key, members)
            else:
                setup_exact(*shapes[members[0]])
    n_rendered = 0
    if a.render_limbs_dir:
        from demo_image import save_image
        from posepaf.render import draw_limbs_records, limb_angle_table_dev
        os.makedirs(a.render_limbs_dir, exist_ok=True)
        limb_angle_table_dev(dev)                   # the device's cos / sin table: built once, outside the timed loop
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    copy_stream = torch.cuda.Stream(device=dev)

    def run_group(members, ragged_key=None):
        """one group through the double-buffered loop.  ragged_key None: every image is (H, W), the equal-size kernels."""
        nonlocal n_rendered
        if ragged_key is None:
            H, W = shapes[members[0]]
            proc = OriginalPathProcessor(post, H, W, B)
        else:   # slots that hold the bucket's largest image and have the padded shape of scale 1
            H, W = padded_shape(max(shapes[k][0] for k in members), max(shapes[k][1] for k in members))
            proc = OriginalPathProcessor(post, None, None, B, slot_area=max(shapes[k][0] * shapes[k][1] for k in members))
            size_index = banks[(ragged_key, "sizes")]
        pinned = [torch.zeros((B, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
        staged = [torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
        canvas = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) if a.render_limbs_dir else None
        events = [None, None]
        batches = [members[b0:b0 + B] for b0 in range(0, len(members), B)]

        def stage(j):   # decode batch j into pinned[j % 2] and start its upload on the copy stream
            if j >= len(batches):
                return
            k = j % 2
            if events[k] is not None:
                events[k][1].synchronize()          # the compute that read staged[k] two batches ago has finished
            view = pinned[k].numpy()

            def put(t):
                if ragged_key is None:
                    view[t[0]] = src.load(int(mine[t[1]]))
                else:
                    h, w = shapes[t[1]]
                    view[t[0], :h, :w] = src.load(int(mine[t[1]]))
            list(pool.map(put, enumerate(batches[j])))
            with torch.cuda.stream(copy_stream):
                staged[k].copy_(pinned[k], non_blocking=True)
                up = torch.cuda.Event()
                up.record(copy_stream)
            events[k] = [up, None]

        stage(0)
        for j, loc in enumerate(batches):
            k = j % 2
            idx = [int(mine[q]) for q in loc]
            n = len(idx)
            torch.cuda.current_stream(dev).wait_event(events[k][0])
            dev_imgs = staged[k]
            slots = torch.tensor([src.scene_slot(i) for i in idx] + [0] * (B - n), dtype=torch.int64, device=dev) if src.has_scenes else None
            with torch.no_grad():
                if ragged_key is None:
                    proc.reset()
                    for sc in scales:
                        scaled = resize_images_u8(dev_imgs, float(sc))
                        sh, sw = scaled.shape[1:3]
                        for ang in angles:
                            m_in, m_rev = input_and_map_inverses(*padded_shape(sh, sw), ang)
                            x = preprocess_batch(scaled, True, torch.float16, m_inv=m_in)
                            ph, pw = x.shape[1:3]
                            maps = model(x).contiguous().view(B, 2, 50, ph // 4, pw // 4)
                            if src.has_scenes:   # the same synthetic people, rendered at this scale (and rotation)
                                maps = torch.addcmul(banks[(H, W, float(sc), ang)].index_select(0, slots), maps, scale)
                            proc.accumulate(maps, ph - sh, pw - sw, n_div, m_inv=m_rev)
                else:   # a short last batch repeats its first image's size in the unused slots (their records are dropped)
                    sizes = [shapes[q] for q in loc] + [shapes[loc[0]]] * (B - n)
                    rg = RaggedBucket(sizes, scales, dev)
                    if src.has_scenes:   # each image's scene comes from the bank of its own (H, W, scale)
                        slots = slots + torch.tensor([size_index[hw] * SCENE_BANK for hw in sizes], dtype=torch.int64, device=dev)
                    proc.reset(rg)
                    for i, sc in enumerate(scales):
                        scaled = resize_images_u8(dev_imgs, float(sc), ragged=rg)
                        ph, pw = scaled.shape[1:3]
                        maps = model(preprocess_ragged(scaled, rg.dev[1 + i], torch.float16)).contiguous().view(B, 2, 50, ph // 4, pw // 4)
                        if src.has_scenes:
                            maps = torch.addcmul(banks[(ragged_key, float(sc))].index_select(0, slots), maps, scale)
                        proc.accumulate(maps, *rg.pads(i), n_div)
                rec = proc.finish(B, thre1)
                if canvas is not None:   # reads staged[k]: before `done`
                    draw_limbs_records(dev_imgs, rec, rg.dev[0] if ragged_key is not None else None, out=canvas)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
            events[k][1] = done
            local.index_copy_(0, torch.tensor(loc, dtype=torch.int64, device=dev), rec.view(B, RECORD_BYTES)[:n])
            stage(j + 1)                            # the next batch is decoded and uploaded while this one computes
            if canvas is not None:   # the canvas is the group's until the next batch's draw: bring it to the host now
                canvases = canvas[:n].cpu().numpy()
                for q, k_local in enumerate(loc):
                    h, w = shapes[k_local]
                    save_image(os.path.join(a.render_limbs_dir, "%06d.%s" % (int(mine[k_local]), a.render_format)), canvases[q, :h, :w])
                    n_rendered += 1

    n_ragged = 0
    for key, members, ragged in groups:
        if not ragged:
            run_group(members)
            continue
        try:
            run_group(members, key)
            n_ragged += 1
        except RaggedUnsupported:   # raised by the bucket's first batch, before any record: its images by exact size instead
            torch.cuda.synchronize()
            for _, sub, _ in group_by_bucket_key([shapes[k] for k in members], scales, exact=True):
                with torch.no_grad():
                    setup_exact(*shapes[members[sub[0]]])
                run_group([members[q] for q in sub])
    torch.cuda.synchronize()
    pool.shutdown(wait=False)
    info = {"launch": "eager", "scales": scales, "decode_threads": workers,
            "original_buckets": {"groups": len(groups), "ragged": n_ragged}}
    if a.rotation_search is not None:
        info["rotation_search"] = angles
    info["test_cfg"] = post.test_cfg      # the configuration in force, read back from the context
    if a.render_limbs_dir:
        info["rendered_files"] = n_rendered
    return local.view(-1), time.perf_counter() - t0, info


# ------------------------------------------------------------------------------------------------ --val_loss
def val_loss_conflicts(a):
    """the options --val_loss cannot be combined with, as the user typed them"""
    named = (("--scales", a.scales is not None), ("--rotation_search", a.rotation_search is not None),
             ("--test_cfg", a.test_cfg is not None), ("--config_file", a.config_file is not None),
             ("--render_dir", a.render_dir is not None), ("--render_limbs_dir", a.render_limbs_dir is not None),
             ("--ap", a.ap is not None), ("--scenes bank", a.scenes_given == "bank"), ("--images", a.images is not None),
             ("--inject_gt", a.inject_gt), ("--gpus", a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1))
    return [name for name, given in named if given]


def segm_mask_stride4(anns_per_image, staged, sizes, dev):
    """--mask_miss segm for one staged batch: the annotations' mask_miss rasterised into the batch's slots (pp_coco_masks_u8) and brought
    to stride 4 by the data transformer under the identity matrix (pp_augment_batch: the 4 x 4 area rule of INTEGRATION section 17; the
    padding around an image reads the border value 255).  staged: device uint8 (B, hp, wp, 3); sizes: device int32 (2, B)
    -> float32 (B, hp / 4, wp / 4), what focal_l2_terms takes as mask"""
    from posepaf import augment, coco_masks
    n, hp, wp, _ = staged.shape
    hw = sizes.cpu().numpy()
    packed = coco_masks.to_device(coco_masks.pack_segmentations(anns_per_image, [(int(hw[0, j]), int(hw[1, j])) for j in range(n)]), dev)
    mask_miss, _ = coco_masks.masks_device(packed, (hp, wp))
    identity = [np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])] * n
    params = torch.from_numpy(augment.pack_params(identity, [False] * n, hp, wp)).to(dev)
    joints = torch.zeros((n, 1, sk.NUM_PART, 3), dtype=torch.float64, device=dev)
    return augment.augment_device(staged, mask_miss, None, sizes, joints, torch.zeros(n, dtype=torch.int32, device=dev), params, (hp, wp))[1]


def run_val_loss(a, src, model, dev):
    """--val_loss: every image through model(x, all_preds=True) and pp_focal_l2_terms against its own device-rendered target.
    -> the meter's summary + seconds (set-up -- tuning the layer shapes of every bucket -- excluded)"""
    import ctypes as C
    from posepaf import _lib, synth_device, val_loss
    L = _lib.load()
    B = a.batch
    segm = getattr(a, "mask_miss", "ones") == "segm"
    # an image with more than one crowd annotation has no mask_miss (the reference's make_mask raises): skipped and counted
    keep = [i for i in range(len(src)) if not segm or sum(s["iscrowd"] == 1 for s in src.segm[src.image_ids[i]]) <= 1]
    if not keep:
        raise SystemExit("--mask_miss segm: every image has more than one crowd annotation")
    groups = {k: [keep[m] for m in members] for k, members in buckets_by_padded_shape([src.shape(i) for i in keep]).items()}
    most = src.max_people(range(len(src)))
    if most > synth_device.MAX_PEOPLE:
        raise SystemExit(f"--val_loss renders at most {synth_device.MAX_PEOPLE} people per image, an image here has {most}")
    meter = val_loss.ValLossMeter()

    def preprocess(staged, sizes):
        n, hp, wp, _ = staged.shape
        x = torch.empty((n, hp, wp, 3), dtype=torch.float16, device=dev)
        _lib.check(L.pp_preprocess_u8_ragged(C.c_void_p(staged.data_ptr()), C.c_void_p(sizes.data_ptr()), C.c_void_p(x.data_ptr()),
                                             _lib.PP_F16, n, hp, wp, sk.PAD_VALUE, 0,
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return x

    with torch.no_grad():
        for (hp, wp), members in groups.items():   # untimed: the kernel choice of every layer shape this bucket runs
            model(torch.zeros((B, hp, wp, 3), dtype=torch.float16, device=dev), all_preds=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for (hp, wp), members in groups.items():
            for b0 in range(0, len(members), B):
                loc = members[b0:b0 + B]
                n = len(loc)                             # a short last batch repeats its first image in the unused slots: one
                loc = loc + [loc[0]] * (B - n)           # batch size per bucket to tune, and the meter counts the first n only
                imgs = np.full((B, hp, wp, 3), sk.PAD_VALUE, np.uint8)
                sizes = np.zeros((2, B), np.int32)
                people = []
                for j, i in enumerate(loc):
                    im = src.load(i)
                    h, w = im.shape[:2]
                    imgs[j, :h, :w] = im
                    sizes[0, j], sizes[1, j] = h, w
                    people.append(src.scene_joints(i, hp, wp))
                joints, n_people = synth_device.pack_joints(people, most)
                staged, sizes_dev = torch.from_numpy(imgs).to(dev), torch.from_numpy(sizes).to(dev)
                x = preprocess(staged, sizes_dev)
                preds = model(x, all_preds=True)
                target = synth_device.render_scenes(torch.from_numpy(joints).to(dev), torch.from_numpy(n_people).to(dev), hp // 4, wp // 4,
                                                    dtype=torch.float16, flip=False, noise=0.0, reverse_kp=True)
                mask = segm_mask_stride4([src.segm[src.image_ids[i]] for i in loc], staged, sizes_dev, dev) if segm else None
                meter.update(val_loss.focal_l2_terms(preds, target, mask=mask), n_valid=n)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
    out = meter.summary()
    out.update({"seconds": dt, "mask_miss": "segm" if segm else "none", "images_per_step": B, "padded_shapes": sorted(groups)})
    if segm:
        out["images_skipped_multi_crowd"] = len(src) - len(keep)
    return out


# ------------------------------------------------------------------------------------------------ --ap host / device
def ground_truth_of(src, indices, original):
    """Ground truth of the images `indices`, as the default report derives it: from the annotation file, or from the injected
    synthetic scene."""
    if src.gts:
        return {src.image_ids[i]: src.gts[src.image_ids[i]] for i in indices if src.image_ids[i] in src.gts}
    gts = {}
    if src.has_scenes:
        for i in indices:
            slot = src.scene_slot(i)
            joints = synth.make_scene_at_scales(src.n_people(slot), 20_000 + slot, [(8, 8, 1.0)], img=src.shape(i)[0])[1] \
                if original else src.joints(slot, *padded_shape(*src.shape(i)))
            gts[src.image_ids[i]] = oks_eval.gt_from_synth_joints(joints)
    return gts


AP_BLOB = (("order", np.int32, 20), ("scores", np.float32, 20), ("match", np.int8, 600), ("n_det", np.int32, 1), ("n_gt", np.int32, 3),
           ("counts", np.int32, 1))


def ap_on_device(src, mine, local_recs, dev, world, backend, S, original):
    """--ap device, every rank: rows + matching of its own records on its own device against its own shard's ground truth, then one
    gather of the per-image outputs (776 bytes of order / scores / flags / counts + the image's result rows).
    -> ({name: array in global image order}, seconds of the ground-truth derivation, seconds of packing + kernels + gather)"""
    from posepaf.ap_device import DeviceKeypointEval
    idx = [int(i) for i in mine]
    t0 = time.perf_counter()
    gts = ground_truth_of(src, idx, original)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    ev = DeviceKeypointEval(dev, [src.image_ids[i] for i in idx], gts)
    out = ev.match(local_recs[: len(idx) * RECORD_BYTES])
    width = torch.zeros(1, dtype=torch.int64, device=dev)
    if len(idx):
        width[0] = out["counts"].max()
    if world > 1:
        import torch.distributed as dist
        width = width if backend == "nccl" else width.cpu()
        dist.all_reduce(width, op=dist.ReduceOp.MAX)
    width = int(width.item())              # rows per image that travel: the most people any image of the set has
    parts = [out[name].reshape(len(idx), n).contiguous().view(torch.uint8) for name, _, n in AP_BLOB]
    parts.append(out["rows"][:, :width].reshape(len(idx), width * 52).contiguous().view(torch.uint8))
    blob = torch.cat(parts, dim=1)
    if world > 1:
        shard = torch.zeros((S, blob.shape[1]), dtype=torch.uint8, device=dev)
        shard[: len(idx)] = blob
        merged = pdist.gather_rows(shard if backend == "nccl" else shard.cpu(), len(idx))
    else:
        merged = blob.cpu().numpy()
    res, at = {}, 0
    for name, dtype, n in AP_BLOB:
        nbytes = n * np.dtype(dtype).itemsize
        res[name] = np.ascontiguousarray(merged[:, at:at + nbytes]).view(dtype).reshape(len(merged), n)
        at += nbytes
    res["rows"] = np.ascontiguousarray(merged[:, at:]).view(np.float32).reshape(len(merged), width, 52)
    res["match"] = res["match"].reshape(len(merged), 3, 10, 20)
    res["n_det"], res["counts"] = res["n_det"].reshape(-1), res["counts"].reshape(-1)
    return res, t1 - t0, time.perf_counter() - t1


def report_with_ap(a, src, merged, summary, gathered, original):
    """rank 0, --ap host / device: results.json, the twelve values and the seconds of each step into `summary`"""
    from posepaf.ap_device import stage_b_inputs
    ids = src.image_ids
    has_gt = bool(src.gts) or src.has_scenes
    key = "keypoint_ap" if src.gts else "synthetic_oks"
    os.makedirs(os.path.dirname(os.path.abspath(a.dump_name)), exist_ok=True)
    if a.ap == "device":
        res, t_gt, t_match = gathered
        t0 = time.perf_counter()
        if has_gt:
            order = sorted(range(len(ids)), key=ids.__getitem__)
            summary[key] = oks_eval.accumulate_ranges(*stage_b_inputs(res["scores"], res["match"], res["n_det"], res["n_gt"], order))
        t1 = time.perf_counter()
        results = []
        rows = res["rows"].astype(np.float64)
        for i, c in enumerate(res["counts"]):
            kps, scores = rows[i, :c, :51].tolist(), rows[i, :c, 51].tolist()
            results.extend({"image_id": ids[i], "category_id": 1, "keypoints": kp, "score": sc} for kp, sc in zip(kps, scores))
        with open(a.dump_name, "w") as f:
            json.dump(results, f)
        t2 = time.perf_counter()
        summary["ap"] = {"path": "device", "seconds_rows_and_match": t_match, "seconds_accumulate": t1 - t0, "seconds_json": t2 - t1,
                         "seconds_ground_truth": t_gt}
    else:
        t0 = time.perf_counter()
        results, dts = [], {}
        for i, rec in enumerate(merged):
            if int(rec["status"]) & 32:      # PP_ST_FLOAT_COORDS (original path): x / y are float32 bit patterns
                rec = rec.copy()
                fx, fy = rec["humans"]["x"].view(np.float32), rec["humans"]["y"].view(np.float32)
                rec["humans"]["x"], rec["humans"]["y"] = np.rint(fx).astype(np.int32), np.rint(fy).astype(np.int32)
            r = coco.coco_results(ids[i], coco.humans_from_record(rec))     # evaluate.py:182-209
            results.extend(r)
            dts[ids[i]] = [{"keypoints": x["keypoints"], "score": x["score"]} for x in r]
        t1 = time.perf_counter()
        gts = ground_truth_of(src, range(len(ids)), original)
        t2 = time.perf_counter()
        per_image = [oks_eval.match_image(gts.get(k, []), dts.get(k, [])) for k in sorted(set(gts) | set(dts))]
        t3 = time.perf_counter()
        if has_gt:
            summary[key] = oks_eval.accumulate_ranges(*oks_eval.concat_matches(per_image))
        t4 = time.perf_counter()
        with open(a.dump_name, "w") as f:
            json.dump(results, f)
        t5 = time.perf_counter()
        summary["ap"] = {"path": "host", "seconds_rows_and_match": (t1 - t0) + (t3 - t2), "seconds_accumulate": t4 - t3,
                         "seconds_json": t5 - t4, "seconds_ground_truth": t2 - t1}
    summary["people_found"] = len(results)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse(argv)
    if a.val_loss:   # a mode of its own: refused combinations leave before anything touches the GPU
        bad = val_loss_conflicts(a)
        if bad:
            raise SystemExit("--val_loss is a mode of its own (the fused model's multi-scale focal-L2 loss against device-rendered "
                             "targets, one process) and does not combine with " + ", ".join(bad))
        if not (a.ann_file or a.synthetic or a.limit):
            raise SystemExit("--val_loss needs images with joints: --synthetic N, or --ann_file F --img_dir D")
        if a.ann_file and not a.img_dir:
            raise SystemExit("--ann_file needs --img_dir")
    if a.mask_miss == "segm" and not (a.val_loss and a.ann_file):
        raise SystemExit("--mask_miss segm rasterises an annotation file's segmentations for --val_loss: it needs --val_loss --ann_file F")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:   # before anything touches the GPU; children are started, never exec'd
        import socket
        import subprocess
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        return subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                                f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
                                os.path.abspath(__file__)] + list(argv), env=env)
    original = not a.run_refactor   # evaluate.py:81-84: predict + find_peaks + find_connections + find_humans
    if original and a.run_cpp:
        raise SystemExit("--run_cpp only exists on the refactored path (evaluate.py:97-129)")
    if not original and any(float(v) != 0.0 for v in (a.rotation_search or [])):
        raise SystemExit("--rotation_search with a non-zero angle runs on the original path only (drop --run_refactor): the "
                         "reference's refactored path returns the last angle's maps alone, rotated about a misplaced centre")
    if a.test_cfg_dict is not None and a.run_cpp:
        raise SystemExit("--test_cfg / --config_file configure the Python rules; the C++ pafprocess rules (--run_cpp) have their "
                         "constants compiled in, as in the reference (utils/pafprocess/pafprocess.h:6-18)")
    if a.test_cfg_dict is not None and not original:
        raise SystemExit("--test_cfg / --config_file run on the original path only (drop --run_refactor): the refactored path's "
                         "captured graphs are built for the INI defaults")
    if a.render_dir is not None and original:
        raise SystemExit("--render_dir draws from the records of the refactored path only (add --run_refactor): the original "
                         "path's ellipse / alpha-blend drawing (demo_image.py:218-240) stays on NumPy in demo_image.py")
    if a.scenes == "device" and original and not a.val_loss:
        raise SystemExit("--scenes device renders one scene per image for the refactored path only (add --run_refactor): the "
                         "original path injects at several scales and angles and keeps its scene banks")
    if a.scenes == "device" and not a.val_loss and not (a.inject_gt or not (a.ann_file or a.images)):
        raise SystemExit("--scenes device needs scenes to render: --synthetic N, or --ann_file with --inject_gt")
    if a.render_limbs_dir is not None and not original:
        raise SystemExit("--render_limbs_dir draws from the records of the original path only (drop --run_refactor): the "
                         "refactored path draws its own style with --render_dir")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "evaluate.py needs MI355X GPUs"
    backend = os.environ.get("POSEPAF_DIST_BACKEND", "nccl")   # "gloo": rehearsal of the N > 1 control flow on fewer GPUs
    local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)      # RCCL over xGMI
        else:
            dist.init_process_group(backend)
    torch.backends.cudnn.benchmark = True

    from config.config import GetConfig, TrainingOpt
    from posepaf.api import PosePostProcessor, records_to_numpy
    from posepaf.fused_model import FusedIMHN
    from posepaf.model_init import build_network

    opt, config = TrainingOpt(), GetConfig(TrainingOpt.config_name)
    try:
        net, _ = build_network(a.arch, a.checkpoint_path, 7)       # evaluate.py:308-309 (strict)
    except ValueError as e:
        raise SystemExit(str(e))
    model = FusedIMHN.from_network(net).eval().to(dev).half().to(memory_format=torch.channels_last)

    # ---- data
    if a.ann_file:
        if not a.img_dir:
            raise SystemExit("--ann_file needs --img_dir")
        src = CocoSource(a.ann_file, a.img_dir, a.all_images, a.limit, a.inject_gt)
    elif a.images:
        src = DirSource(a.images, a.limit)
    else:
        sizes = [tuple(int(v) for v in t.lower().split("x")) for t in a.sizes.split(",")]
        src = SyntheticSource(a.limit or a.synthetic, sizes, a.people, noise=a.scene_noise, per_image=a.scenes == "device" or a.val_loss)
    n_images = len(src)
    if n_images == 0:
        raise SystemExit("nothing to evaluate: pass --ann_file F --img_dir D, --images DIR or --synthetic N")

    if a.val_loss:
        summary = run_val_loss(a, src, model, dev)
        summary["arch"] = a.arch
        print(json.dumps(summary))
        return 0
    scales = a.scales or [1.0]
    mine = pdist.shard_indices(n_images, rank, world)
    S = pdist.padded_shard_size(n_images, world)
    all_shapes = [src.shape(int(i)) for i in (range(n_images) if n_images <= 200_000 else mine)]
    hp = max(padded_shape(h, w)[0] for h, w in all_shapes) // 4
    wp = max(padded_shape(h, w)[1] for h, w in all_shapes) // 4
    # feature maps up to hp x wp (area bound).  With the C++ rules a map that does not fit LDS stays in device memory (the
    # large-map kernels, up to 650 x 950); the Python rules refuse such a map, loudly
    post = PosePostProcessor(max_batch=a.batch, max_h=hp if not original else int(hp * max(scales) + 16),
                             max_w=wp if not original else int(wp * max(scales) + 16), max_peaks_per_part=64, device=local)
    if original:
        local_recs, dt_local, info = run_original(a, src, mine, model, post, dev)
    else:
        local_recs, dt_local, info = run_refactored(a, src, mine, model, post, dev, rank, world)

    if world > 1:
        import torch.distributed as dist
        shard = torch.zeros(S * RECORD_BYTES, dtype=torch.uint8, device=dev)
        shard[: len(mine) * RECORD_BYTES] = local_recs[: len(mine) * RECORD_BYTES]
        merged = pdist.gather_records(shard if backend == "nccl" else shard.cpu(), len(mine))
        t = torch.tensor([dt_local], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        if "rendered_files" in info:    # every rank wrote its own images
            n = torch.tensor([info["rendered_files"]], dtype=torch.int64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(n, op=dist.ReduceOp.SUM)
            info["rendered_files"] = int(n.item())
    else:
        merged = records_to_numpy(local_recs[:len(mine) * RECORD_BYTES])
        dt = dt_local

    gathered = ap_on_device(src, mine, local_recs, dev, world, backend, S, original) if a.ap == "device" else None
    if rank == 0 and a.ap is not None:
        summary = {"images": int(n_images), "world": world, "images_per_sec": n_images / dt, "seconds": dt,
                   "images_per_gpu_per_step": a.batch, "rules": "original" if original else ("cpp" if a.run_cpp else "python"),
                   "people_found": 0,
                   "status_or": int(np.bitwise_or.reduce(merged["status"])) if len(merged) else 0}
        if summary["status_or"] & 128:
            summary["recon_undefined_images"] = int(np.count_nonzero(merged["status"] & 128))
        summary.update(info)
        report_with_ap(a, src, merged, summary, gathered, original)
        print(json.dumps(summary, default=str))
    elif rank == 0:
        results, dts, gts = [], {}, dict(src.gts)
        for i, rec in enumerate(merged):
            if int(rec["status"]) & 32:      # PP_ST_FLOAT_COORDS (original path): x / y are float32 bit patterns
                rec = rec.copy()
                fx, fy = rec["humans"]["x"].view(np.float32), rec["humans"]["y"].view(np.float32)
                rec["humans"]["x"], rec["humans"]["y"] = np.rint(fx).astype(np.int32), np.rint(fy).astype(np.int32)
            humans = coco.humans_from_record(rec)
            res = coco.coco_results(src.image_ids[i], humans)     # evaluate.py:182-209
            results.extend(res)
            dts[src.image_ids[i]] = [{"keypoints": r["keypoints"], "score": r["score"]} for r in res]
            if src.has_scenes and not src.gts:
                slot = src.scene_slot(i)
                joints = synth.make_scene_at_scales(src.n_people(slot), 20_000 + slot, [(8, 8, 1.0)], img=src.shape(i)[0])[1] \
                    if original else src.joints(slot, *padded_shape(*src.shape(i)))
                gts[src.image_ids[i]] = oks_eval.gt_from_synth_joints(joints)
        os.makedirs(os.path.dirname(os.path.abspath(a.dump_name)), exist_ok=True)
        with open(a.dump_name, "w") as f:
            json.dump(results, f)
        summary = {"images": int(n_images), "world": world, "images_per_sec": n_images / dt, "seconds": dt,
                   "images_per_gpu_per_step": a.batch, "rules": "original" if original else ("cpp" if a.run_cpp else "python"),
                   "people_found": len(results),
                   "status_or": int(np.bitwise_or.reduce(merged["status"])) if len(merged) else 0}
        if summary["status_or"] & 128:   # PP_ST_RECON_UNDEFINED: remove_recon met a case where the reference itself raises
            summary["recon_undefined_images"] = int(np.count_nonzero(merged["status"] & 128))
        summary.update(info)
        if gts:
            key = "keypoint_ap" if src.gts else "synthetic_oks"     # ground truth from the annotation file / from the injected scenes
            summary[key] = oks_eval.evaluate_keypoints(gts, dts)
        print(json.dumps(summary, default=str))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
