#!/usr/bin/env python3
"""Substitute the @PLACEHOLDER@ numbers of DESIGN.md / README.md from the bench lines kept under profiles/ (round 3) and the
tables of DESIGN section 6, rounds 27 and 28, from the probes' JSON (numbers only: the prose lives in the templates).
Idempotent: the templates live in DESIGN.md.in / README.md.in next to the outputs."""
import json
import os
import re
import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line(name):
    return json.loads(open(os.path.join(ROOT, "profiles", name)).read().strip().splitlines()[-1])


d, m = line("r03_bench_default_b128.json"), line("r03_bench_multiscale_b32.json")
kb = d["kernel_ms"]["k_limb_connect"] * 1e3
vals = {
    "E2E": f"{d['value']:.0f}", "E2EMS": f"{d['ms_per_step']:.1f}", "MS": f"{m['value']:.0f}",
    "KB": f"{kb:.0f}", "KBFRAC": f"{d['roofline']['frac']:.2f}",
    "CHAIN": f"{d['roofline']['chain']['ms'] * 1e3:.0f}", "KA": f"{d['kernel_ms']['k_heat_peaks'] * 1e3:.0f}",
    "CHAINFRAC": f"{d['roofline']['chain']['frac']:.2f}",
    "FWD": f"{d['roofline_forward']['achieved']:.0f}", "FWDFRAC": f"{d['roofline_forward']['frac']:.3f}",
    "OWN": str(d["conv_layers"]["shapes_own_kernel"]), "CK": str(d["conv_layers"]["shapes_ck_template_kernel"]),
    "MSFWD": f"{m['roofline_forward']['frac']:.2f}", "CPU": f"{d['cpu_baseline']['value']:.0f}",
    "CPU1": f"{d['cpu_baseline']['single_core']['value']:.1f}",
}


def round27():
    """the tables of DESIGN section 6, round 27, from profiles/r27_conv_dgrad.json (tools/conv_dgrad_probe.py)"""
    doc = json.load(open(os.path.join(ROOT, "profiles", "r27_conv_dgrad.json")))
    span = lambda r, u, f: f"{r['median_' + u]:{f}} ({r['min_' + u]:{f}} – {r['max_' + u]:{f}})"
    rows = []
    for side, r in doc["kernel"].items():
        k, t = r["pp_conv3x3_dgrad_f16"], r["torch conv2d_input, binary16"]
        rows.append(f"| {side.split('x')[0]}² | {r['m']} | {span(k, 'us', '.1f')} | {k['floor_us_at_8TBs']:.1f} | {k['useful_tflops']:.1f} | {span(t, 'us', '.1f')} |")
    step = doc["step"]
    srows = [f"| `train=\"{m}\"` | {step[m]['median_ms_per_step']:.2f} | {step[m]['min_ms_per_step']:.2f} – {step[m]['max_ms_per_step']:.2f} | "
             f"{step[m]['graph_replays']} | {step[m]['skipped_steps']} |" for m in ("heads", "heads+conv", "heads+conv2")]
    add = step["heads+conv2"]["median_ms_per_step"] - step["heads+conv"]["median_ms_per_step"]
    dg = sum(r["pp_conv3x3_dgrad_f16"]["median_us"] for r in doc["kernel"].values()) / 1e3
    wg = sum(r["pp_conv3x3_wgrad_f16"]["median_us"] for r in
             json.load(open(os.path.join(ROOT, "profiles", "r26_conv_wgrad.json")))["kernel"].values()) / 1e3
    cmp = doc["against_the_parent_commit"]
    prows = [f"| `train=\"{mode}\"` | {span(cmp[mode]['this'], 'ms_per_step', '.2f')} | {span(cmp[mode]['parent'], 'ms_per_step', '.2f')} | "
             f"{'yes' if cmp[mode]['this_median_inside_the_parents_range'] else 'no'} |" for mode in ("heads", "heads+conv")]
    procs = [f"| {i} | {r['version']} | " + " | ".join(f"{statistics.median(r['ms_per_step'][m]):.2f} ({min(r['ms_per_step'][m]):.2f} – "
                                                        f"{max(r['ms_per_step'][m]):.2f})" for m in ("heads", "heads+conv"))
             + f" | {r['kernel_choices']['hash']} ({r['kernel_choices']['entries']}) |" for i, r in enumerate(cmp["processes"])]
    return {"R27KERNEL": "\n".join(rows), "R27STEP": "\n".join(srows), "R27ADD": f"{add:.2f}", "R27DG": f"{dg:.2f}", "R27WG": f"{wg:.2f}",
            "R27ACC": f"{4 * (dg + wg):.1f}", "R27PARENT": "\n".join(prows), "R27PROCESSES": "\n".join(procs)}


def round28():
    """the tables of DESIGN section 6, round 28, from profiles/r28_helper_tests.json (the pytest logs of the built library and of each
    mutated one, tests/test_gpu_helper_kernels.py with the two older helper tests of tests/test_gpu_model.py)"""
    doc = json.load(open(os.path.join(ROOT, "profiles", "r28_helper_tests.json")))
    names = lambda d: ", ".join(f"`{k}` ({v})" for k, v in d.items()) or "—"
    rows = [f"| {m['edit']} | {names(m['old_tests_failed'])} | {names(m['new_tests_failed'])} |" for m in doc["mutants"].values()]
    real = doc["real"]
    bounds = "\n".join(f"| {k} | {v:.4f} |" for k, v in real["err_over_bound"].items())
    return {"R28MUT": "\n".join(rows), "R28BOUND": bounds, "R28WALL": f"{real['wall_s']:.1f}", "R28PASSED": str(real["passed"]),
            "R28SLOWEST": f"{float(real['slowest'][0][0]):.1f}"}


vals.update(round27())
vals.update(round28())
for name in ("DESIGN.md", "README.md"):
    src = os.path.join(ROOT, name + ".in")
    if not os.path.exists(src):
        continue
    text = open(src).read()
    text = re.sub(r"@([A-Z0-9]+)@", lambda mo: vals.get(mo.group(1), mo.group(0)), text)
    left = re.findall(r"@[A-Z0-9]+@", text)
    assert not left, left
    open(os.path.join(ROOT, name), "w").write(text)
    print(name, "written")
