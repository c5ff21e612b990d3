#!/usr/bin/env python3
"""Generate tests/golden/g7_cfg_*.npz + g7_cfg_index.json: the REFERENCE's own Python post-processing under non-default
test configurations (run in the build container only, like make_golden.py, whose import machinery this reuses).

    python tests/golden/make_golden_cfg.py

For every configuration of CONFIGS (one per key moved off its INI default, mid_num below 8 and above 20, remove_recon = 1,
and one with everything moved) it stores

* refactored-path inputs (what pp_process_batch_py sees): for the scenes of scenes.json plus the extra crowded scenes listed
  in EXTRA_SCENES, the reference's find_connections + find_humans on the oracle's refined peaks and x4 limb maps
  (`<scene>__py_persons`, `<scene>__py_n_connections`), exactly as make_golden.py does for the defaults;
* original-path inputs (what OriginalPathProcessor.finish sees): for ORIGINAL_SCENES, maps from oracle.predict_accumulate
  on synth.make_scene_at_scales (bit-equal to the GPU accumulators, tests/test_gpu_parity.py), peaks by the reference's
  keypoint_heatmap_nms + refine_centroid(offset_radius) looped as find_peaks (:298-319) does, then the reference's
  find_connections / find_humans on the float64 maps (`<scene>__o_rows`, `__o_persons`, `__o_n_connections`).

Only results and settings are stored; inputs are regenerated from posepaf.synth and SHA-checked (g7_cfg_index.json).

Conditions asserted here, so that a test cannot pass by never reaching the new code:
* every configuration changes the reference's output on at least one stored scene relative to the defaults;
* at least one stored scene takes the remove_recon deletion (:559-564), i.e. differs from remove_recon = 0 on the same
  connections (the index records which);
* no stored (scene, configuration) makes the reference raise.
"""
import hashlib
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import numpy as np  # noqa: E402

DEFAULTS = {"thre1": 0.1, "thre2": 0.1, "connect_ration": 0.8, "mid_num": 20, "len_rate": 16.0, "connection_tole": 0.7,
            "offset_radius": 2, "remove_recon": 0}
CONFIGS = {
    "thre2": {"thre2": 0.3},
    "connect_ration": {"connect_ration": 0.95},
    "mid_num_5": {"mid_num": 5},
    "mid_num_40": {"mid_num": 40},
    "mid_num_100": {"mid_num": 100},
    "len_rate": {"len_rate": 1.25},
    "connection_tole": {"connection_tole": 1.6},
    "offset_radius_0": {"offset_radius": 0},
    "offset_radius_4": {"offset_radius": 4},
    "thre1": {"thre1": 0.3},
    "remove_recon": {"remove_recon": 1},
    "all_moved": {"thre1": 0.15, "thre2": 0.05, "connect_ration": 0.7, "mid_num": 33, "len_rate": 2.0, "connection_tole": 1.2,
                  "offset_radius": 3, "remove_recon": 1},
}
# keys that only the original path reads (find_peaks): the refactored-path scenes cannot show a change for them
ORIGINAL_ONLY = {"thre1", "offset_radius"}
# crowded / noisy scenes built as tests/test_gpu_parity.py::test_assembly_stress_crowded_and_noisy_scenes builds them,
# searched for one that reaches the remove_recon deletion (see find_recon_scenes); (P, seed, noise, dtype)
EXTRA_SCENES = []   # filled by find_recon_scenes when the scenes of scenes.json do not reach the branch
ORIGINAL_SCENES = [(3, 324, "f16"), (8, 329, "f32")]     # (people, seed, dtype): the existing original-path test's scenes
ORIGINAL_SIZES = [(32, 32, 0.5), (64, 64, 1.0), (96, 96, 1.5)]
ORIGINAL_IMG = 256


def cfg_of(moved):
    c = dict(DEFAULTS)
    c.update(moved)
    return c


def main():
    warnings.simplefilter("ignore", DeprecationWarning)   # int(np.where(...)[0]) on a one-element array (NumPy >= 1.25)
    ps, util, cfgmod = mg.import_reference()
    sys.path.append(mg.ROOT)
    sys.path.append(mg.PKG)
    import torch
    from oracle.oracle import Oracle
    from posepaf import synth
    config = cfgmod.GetConfig("Canonical")
    limbs = np.asarray(config.limbs_conn)
    orc = Oracle()

    def refactored_inputs(P, seed, dt, noise=0.02):
        net = synth.make_net_output(P, seed, noise=noise, dtype=np.float16 if dt == "f16" else np.float32)
        heat, paf = orc.flip_average(net)
        jl, _ = orc.heatmap_nms(heat)
        up = orc.upsample4_hwc(paf)
        all_peaks = [[tuple(float(v) for v in row[:4]) for row in jl[jl[:, 4] == k]] for k in range(18)]
        return net, all_peaks, up

    def run_py(all_peaks, paf_hwc, img_h, c):
        conn, special = ps.find_connections(all_peaks, paf_hwc, img_h, c, limbs)
        persons, _ = ps.find_humans(conn, special, all_peaks, c, limbs)
        return (np.asarray(persons, np.float64).reshape(-1, 20, 2), np.array([len(x) for x in conn], np.int32)), (conn, special)

    def reaches_deletion(all_peaks, conn, special):
        try:
            a, _ = ps.find_humans(conn, special, all_peaks, cfg_of({"remove_recon": 1}), limbs)
            b, _ = ps.find_humans(conn, special, all_peaks, cfg_of({}), limbs)
        except Exception:
            return False
        return not np.array_equal(np.asarray(a), np.asarray(b))

    scenes = {k: (v["P"], v["seed"], v["dtype"], 0.02) for k, v in json.load(open(os.path.join(HERE, "scenes.json"))).items()}
    inputs = {k: refactored_inputs(P, seed, dt, noise) for k, (P, seed, dt, noise) in scenes.items()}
    base = {k: run_py(ap, up, 512, cfg_of({})) for k, (_, ap, up) in inputs.items()}
    recon_scenes = [k for k in scenes if reaches_deletion(inputs[k][1], *base[k][1])]
    if not recon_scenes:   # search seeded crowded scenes, as the stress test builds them, for one that reaches the branch
        for people, noise in [(12, 0.04), (22, 0.03), (33, 0.04), (45, 0.02)]:
            for i in range(8):
                P, seed, dt = people, 7000 + 13 * people + i, ("f16" if i % 2 else "f32")
                net, ap, up = refactored_inputs(P, seed, dt, noise)
                try:
                    res = run_py(ap, up, 512, cfg_of({}))
                except Exception:
                    continue
                if reaches_deletion(ap, *res[1]):
                    key = f"P{P}_s{seed}_{dt}_n{noise}"
                    scenes[key], inputs[key], base[key] = (P, seed, dt, noise), (net, ap, up), res
                    recon_scenes.append(key)
                    EXTRA_SCENES.append((P, seed, noise, dt))
                    break
            if recon_scenes:
                break
    assert recon_scenes, "no scene reaches the remove_recon deletion; widen the search"
    print("remove_recon deletion reached by:", recon_scenes)

    # original-path inputs
    o_inputs = {}
    for people, seed, dt in ORIGINAL_SCENES:
        outs, _ = synth.make_scene_at_scales(people, seed, ORIGINAL_SIZES, dtype=np.float16 if dt == "f16" else np.float32,
                                             img=ORIGINAL_IMG)
        heat = np.zeros((20, ORIGINAL_IMG, ORIGINAL_IMG))
        paf = np.zeros((30, ORIGINAL_IMG, ORIGINAL_IMG))
        for o in outs:
            orc.predict_accumulate(o, 0, 0, ORIGINAL_IMG, ORIGINAL_IMG, len(ORIGINAL_SIZES), heat, paf)
        sha = hashlib.sha256(b"".join(np.ascontiguousarray(o).tobytes() for o in outs)).hexdigest()
        o_inputs[f"O{people}_s{seed}_{dt}"] = (heat, paf, sha, (people, seed, dt))

    def run_original(heat, paf, c):
        # find_peaks, utils/parse_skeletons.py:286-321, with the .cuda() of :296 left out (CPU tensor)
        hm = np.ascontiguousarray(heat.transpose(1, 2, 0)).astype(np.float32)
        fm = torch.from_numpy(hm[:, :, :18].copy().transpose((2, 0, 1))[None, ...])
        fm = util.keypoint_heatmap_nms(fm, kernel=3, thre=c["thre1"]).numpy().squeeze().transpose((1, 2, 0))
        all_peaks, counter = [], 0
        for part in range(18):
            map_orig = hm[:, :, part]
            py_, px_ = np.nonzero(fm[:, :, part])
            peaks = list(zip(px_, py_))
            refined = [util.refine_centroid(map_orig, anchor, c["offset_radius"]) for anchor in peaks]
            ids = range(counter, counter + len(refined))
            all_peaks.append([refined[i] + (ids[i],) for i in range(len(ids))])
            counter += len(peaks)
        (persons, ncn), _ = run_py(all_peaks, np.ascontiguousarray(paf.transpose(1, 2, 0)), ORIGINAL_IMG, c)
        rows = np.array([tuple(float(v) for v in pk) + (float(part),) for part, pks in enumerate(all_peaks) for pk in pks],
                        np.float64).reshape(-1, 5)
        return rows, persons, ncn

    o_base = {k: run_original(h, p, cfg_of({})) for k, (h, p, _, _) in o_inputs.items()}

    index = {"defaults": DEFAULTS, "configs": {}, "recon_scenes": recon_scenes,
             "scenes": {k: {"P": P, "seed": seed, "dtype": dt, "noise": noise,
                            "net_sha256": hashlib.sha256(inputs[k][0].tobytes()).hexdigest()}
                        for k, (P, seed, dt, noise) in scenes.items()},
             "original_scenes": {k: {"people": m[0], "seed": m[1], "dtype": m[2], "sizes": ORIGINAL_SIZES, "img": ORIGINAL_IMG,
                                     "outs_sha256": sha} for k, (_, _, sha, m) in o_inputs.items()}}
    for name, moved in CONFIGS.items():
        c = cfg_of(moved)
        store, changed = {}, []
        if not set(moved) <= ORIGINAL_ONLY:
            for k, (_, ap, up) in inputs.items():
                (persons, ncn), _ = run_py(ap, up, 512, c)   # a raise here fails the generation: no stored scene may raise
                store[f"{k}__py_persons"], store[f"{k}__py_n_connections"] = persons, ncn
                if not (np.array_equal(persons, base[k][0][0]) and np.array_equal(ncn, base[k][0][1])):
                    changed.append(k)
        for k, (heat, paf, _, _) in o_inputs.items():
            rows, persons, ncn = run_original(heat, paf, c)
            store[f"{k}__o_rows"], store[f"{k}__o_persons"], store[f"{k}__o_n_connections"] = rows, persons, ncn
            b = o_base[k]
            if not (np.array_equal(rows, b[0]) and np.array_equal(persons, b[1]) and np.array_equal(ncn, b[2])):
                changed.append(k)
        assert changed, f"configuration {name} changes nothing on the stored scenes: pick a stronger value"
        if moved.get("remove_recon"):
            assert any(k in changed for k in recon_scenes), f"{name}: the deletion scene does not differ"
        index["configs"][name] = {"moved": moved, "changed": changed}
        np.savez_compressed(os.path.join(HERE, f"g7_cfg_{name}.npz"), **store)
        print(name, "changes", changed)
    with open(os.path.join(HERE, "g7_cfg_index.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
