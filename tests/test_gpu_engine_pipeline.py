"""GPU: the pipelined loop of posepaf/engine.py -- pinned slots filled by producer threads, uploads on a copy stream into a
two-deep staging ring, one captured graph per (Hp, Wp, b) plan in one shared memory pool, one post-processing context for all
plans, short tails on smaller plans, records scattered without a synchronisation -- against a run of every image ALONE,
synchronously, through entry points the engine does not use (the equal-size pre-processing kernel, the model at batch 1,
PosePostProcessor.process at max_batch = 1 with a scalar height).

The property: the maps and the record of an image depend on that image alone -- not on its batch neighbours, its position, its
plan's batch size, what the slot held before, the order of the jobs or how far uploads run ahead of compute.  Maps are compared
bit for bit, records with test_gpu_parity._same_record; the one-image run itself is anchored to the oracle.

Cases: tests/engine_cases.py (66 images, three padded shapes, five plans, two passes of six jobs in opposite orders = 12 submits
and one synchronisation); tests/test_engine_cases_cpu.py pins that these cases can show a fault.

The device-side sleep of the two held-back variants: SLEEP_CYCLES below.
"""
import time

import numpy as np
import pytest

import engine_cases as ec
from test_gpu_parity import SCORE_TOL, _records_vs_oracle, _same_record

pytestmark = pytest.mark.gpu

# torch.cuda._sleep(SLEEP_CYCLES) in front of a pass holds one stream back while the host enqueues the pass.  Measured on the
# MI355X (this engine, graph replay, the six jobs of a pass with their slot fills, time.perf_counter around the acquire / fill /
# submit loop, nothing held back): 1.7 to 2.6 ms per pass over ten passes; torch.cuda._sleep lasts 0.4165 ms per million cycles
# (0.417 / 4.135 / 41.65 ms for 1e6 / 1e7 / 1e8).  Chosen: four times the slowest pass = 10.4 ms = 25 million cycles (the cap of
# 200 ms per pass is far away).  Fixed from that measurement, not from what the tests below give.
MEASURED_ENQUEUE_MS = 2.6
MEASURED_MS_PER_MCYCLE = 0.4165
SLEEP_CYCLES = 25_000_000


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    return ec.TinyModel(torch_cuda)


@pytest.fixture(scope="module")
def post(torch_cuda):
    """the ONE post-processing context every engine and every plan of this module shares"""
    from posepaf.api import PosePostProcessor
    p = PosePostProcessor(max_batch=ec.B, max_h=32, max_w=48, max_peaks_per_part=64)
    yield p
    del _ALIVE[:]
    p.close()


@pytest.fixture(scope="module")
def banks(torch_cuda):
    return {k: torch_cuda.from_numpy(ec.bank(k).copy()).cuda() for k in "ABC"}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


class _Alone:
    """every image by itself: crop -> pp_preprocess_u8 (equal-size kernel) -> model at batch 1 -> scene + 1e-3 * output ->
    process / process_py with the image's own height as a scalar; synchronous"""

    def __init__(self, torch, model, scene_of):
        from posepaf.api import PosePostProcessor
        self.torch, self.model, self.scene_of = torch, model, scene_of
        self.post1 = PosePostProcessor(max_batch=1, max_h=32, max_w=48, max_peaks_per_part=64)
        self.scale = torch.tensor(ec.INJECT_SCALE, dtype=torch.float16, device="cuda")

    def maps(self, i, im):
        from posepaf import pipeline
        torch = self.torch
        hp, wp = ec.PADDED[ec.bucket(i)]
        x = pipeline.preprocess_batch(torch.from_numpy(np.array(im)).cuda()[None], True, torch.float16)
        assert tuple(x.shape) == (2, hp, wp, 3)
        out = self.model(x).view(1, 2, 50, hp // 4, wp // 4)
        return torch.addcmul(self.scene_of(i), out, self.scale)

    def run(self, rules):
        """-> ([maps (2, 50, h4, w4) float16 on the host], {rule: [record]})"""
        maps, recs = [], {r: [] for r in rules}
        for i in range(ec.N_IMAGES):
            im = ec.image(i)
            m = self.maps(i, im)
            for r in rules:
                fn = self.post1.process if r == "cpp" else self.post1.process_py
                recs[r].append(fn(m, im.shape[0])[0].copy())
            maps.append(m.cpu().numpy()[0])
        return maps, recs

    def close(self):
        self.post1.close()


def _anchor_cpp(oracle, maps, recs, what):
    """the one-image records against the oracle's whole path on the same maps -> images left out (undefined sort in the oracle)"""
    left_out = []
    for i in range(ec.N_IMAGES):
        want = oracle.pipeline(maps[i], ec.shapes()[i][0])
        assert bool(recs[i]["status"] & 8) == bool(want["sort_oob"]), (what, i)      # PP_ST_SORT_UNDEFINED where the oracle sees it
        if want["sort_oob"]:
            left_out.append(i)
            continue
        assert recs[i]["status"] == 0, (what, i, hex(int(recs[i]["status"])))
        _records_vs_oracle(recs[i], want, f"{what}: image {i} alone")
    print(f"{what}: {len(left_out)} of {ec.N_IMAGES} images left out of the oracle anchor (undefined sort): {left_out}")
    return left_out


def _anchor_py(oracle, maps, recs):
    for i in range(ec.N_IMAGES):
        heat, paf = oracle.flip_average(maps[i])
        jl, _ = oracle.heatmap_nms(heat)
        persons, ncn = oracle.py_find_humans(jl, oracle.upsample4_hwc(paf), ec.shapes()[i][0])
        rec = recs[i]
        n = int(rec["n_humans"])
        assert n == len(persons) and rec["n_connections"] == int(ncn.sum()) and rec["n_peaks"] == len(jl), i
        assert np.array_equal(rec["humans"]["peak_id"][:n], persons[:, :18, 0].astype(np.int32)), i
        assert np.allclose(rec["humans"]["score"][:n], persons[:, 18, 0] / persons[:, 19, 0], rtol=0, atol=SCORE_TOL), i


@pytest.fixture(scope="module")
def truth(torch_cuda, model, banks, oracle):
    """bank scenes: {"maps": [...], "cpp": [...], "py": [...]} of the 66 images, each alone; computed once, never changed"""
    torch = torch_cuda
    # the premise of everything below: the stand-in network gives an image the same bits at any batch size and position
    g = torch.Generator().manual_seed(8)
    x = torch.rand((2 * ec.B, 128, 128, 3), generator=g).half().cuda()
    whole = model(x)
    assert tuple(whole.shape) == (2 * ec.B, 50, 32, 32) and whole.dtype == torch.float16
    for j in range(2 * ec.B):
        assert torch.equal(whole[j:j + 1], model(x[j:j + 1])), \
            f"WRONG TEST PREMISE (not an engine defect): the stand-in model's output for entry {j} depends on the batch size"
    alone = _Alone(torch, model, lambda i: banks[ec.bucket(i)][ec.scene_index(i)][None])
    try:
        maps, recs = alone.run(("cpp", "py"))
        # one grey level at one pixel inside the corner shows in the maps (the pixel is chosen by engine_cases.sensitive_pixel)
        y, x_, col, new = ec.sensitive_pixel(0, maps[0])
        im = ec.image(0).copy()
        assert abs(int(im[y, x_, col]) - new) == 1
        im[y, x_, col] = new
        changed = int((_bits(alone.maps(0, im).cpu().numpy()[0]) != _bits(maps[0])).sum())
        print(f"one grey level at pixel ({y}, {x_}, {col}) of image 0 changes {changed} map elements")
        assert changed >= 1
    finally:
        alone.close()
    assert all(int(r["n_humans"]) >= 1 for r in recs["cpp"])
    left_out = _anchor_cpp(oracle, maps, recs["cpp"], "bank scenes")
    assert len(left_out) <= 2
    _anchor_py(oracle, maps, recs["py"])
    for m in maps:
        m.setflags(write=False)
    return {"maps": maps, "cpp": recs["cpp"], "py": recs["py"]}


@pytest.fixture(scope="module")
def truth_device(torch_cuda, model, oracle):
    """scenes="device": every image's own scene from render_scenes at batch 1 with the engine's seed and the image's scene id"""
    from posepaf import synth_device
    torch = torch_cuda

    def scene_of(i):
        hp, wp = ec.PADDED[ec.bucket(i)]
        joints, n = synth_device.pack_joints([ec.people(i)], ec.DEVICE_MAX_PEOPLE)
        return synth_device.render_scenes(torch.from_numpy(joints).cuda(), torch.from_numpy(n).cuda(), hp // 4, wp // 4, torch.float16,
                                          flip=True, noise=ec.DEVICE_NOISE, seed=ec.DEVICE_SEED,
                                          scene_ids=torch.tensor([i], dtype=torch.int64, device="cuda"))
    alone = _Alone(torch, model, scene_of)
    try:
        maps, recs = alone.run(("cpp",))
    finally:
        alone.close()
    _anchor_cpp(oracle, maps, recs["cpp"], "device scenes")
    assert sum(int(r["n_humans"]) >= 1 for r in recs["cpp"]) >= ec.N_IMAGES * 3 // 4
    return {"maps": maps, "cpp": recs["cpp"]}


# ------------------------------------------------------------------------------------------------ the pipelined side
# Every engine of this module stays alive until the module is done.  Destroying a plan's captured graph waits for the device,
# so an engine that goes away while a later test holds a stream back would make the host sit out the sleep, and that test's
# pass would be enqueued with nothing held back (seen on the MI355X: the release of one stale _Plan cost the whole sleep).
_ALIVE = []


def make_engine(torch, model, post, banks, rules="cpp", use_graph=True, plan_keys=None, **kw):
    """an engine with every plan of the job list prepared, and every pinned slot filled with the poison pattern"""
    from posepaf.engine import InferenceEngine
    eng = InferenceEngine(model, post, ec.B, 0, rules=rules, use_graph=use_graph, inject_scale=ec.INJECT_SCALE,
                          max_image_hw=ec.MAX_IMAGE_HW, **kw)
    assert len(eng.slots) == 3 and len(eng.staging) == 2              # the defaults the variants below are laid out for
    label_of = {v: k for k, v in ec.PADDED.items()}
    for key in plan_keys or sorted({key for key, _ in ec.make_jobs(ec.shapes())}):
        plan = eng.plan(*key)
        if eng.scenes == "bank":
            eng.set_bank(plan, banks[label_of[key[:2]]])
    for plan in eng.plans.values():
        eng.prepare(plan)
        assert (plan.graph is not None) == use_graph
    eng.sync()
    pattern = ec.poison(eng.max_bytes)
    assert (pattern != 128).all()                                     # the pad value: a leak of it would be no leak at all
    for slot in eng.slots:
        slot.np[:] = pattern
    _ALIVE.append(eng)
    return eng


def make_fill(device_scenes=False):
    """evaluate.py's fill(): the image into its own corner only, its sizes, its bank index (or its people and scene id)"""
    def fill(i, j, sizes, idx, imgs, n_people=None, joints=None):
        im = ec.image(i)
        h, w = im.shape[:2]
        imgs[j, :h, :w] = im
        sizes[0, j], sizes[1, j] = h, w
        if device_scenes:
            pj = ec.people(i)
            p = pj.shape[0]
            joints[j, :p] = pj
            joints[j, p:, :, 2] = 2
            n_people[j] = p
            idx[j] = i
        else:
            idx[j] = ec.scene_index(i)
    return fill


class _Taken:
    """device copies of what a plan holds after a job, enqueued on the compute stream before the next submit"""

    def __init__(self, render=False):
        self.render, self.jobs = render, []

    def __call__(self, plan, loc):
        self.jobs.append(((plan.hp, plan.wp, plan.b), list(loc), plan.maps.clone(), plan.records.clone(),
                          plan.canvas.clone() if self.render else None))


def run_product_loop(torch, eng, job_lists, device_scenes=False, render=False):
    """engine.run_jobs, the loop evaluate.py runs, over all passes in one go; one synchronisation at the end"""
    from posepaf._lib import RECORD_BYTES
    from posepaf.engine import run_jobs
    jobs = [(eng.plan(*key), loc) for one in job_lists for key, loc in one]
    out = torch.zeros((ec.N_IMAGES, RECORD_BYTES), dtype=torch.uint8, device=eng.dev)
    taken = _Taken(render)
    run_jobs(eng, jobs, make_fill(device_scenes), out, workers=4, depth=2, on_batch=taken)
    eng.sync()
    return taken, out


PROBE_CYCLES = 5_000_000      # about 2 ms: long against the few microseconds the host needs to enqueue the probe's copy


def _overlaps(torch, held, other):
    """True when a small upload on `other` completes while `held` sleeps.  Streams are spread over a few hardware queues
    (HIP's GPU_MAX_HW_QUEUES, 4 by default); two that share one run strictly one after the other, and between such a pair no
    stream can be held back while the other runs ahead."""
    host = torch.zeros(4096, dtype=torch.uint8).pin_memory()
    dev = torch.empty(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(held):
        torch.cuda._sleep(PROBE_CYCLES)
        end = torch.cuda.Event()
        end.record(held)
    with torch.cuda.stream(other):
        dev.copy_(host, non_blocking=True)
        done = torch.cuda.Event()
        done.record(other)
    done.synchronize()
    ahead = not end.query()
    torch.cuda.synchronize()
    return ahead


def compute_stream_beside(torch, eng):
    """a compute stream that really runs beside the engine's copy stream, in both directions: the current stream if it does,
    else the first of a few fresh ones that does (the engine computes on whatever stream is current at submit)"""
    tried = []
    for n in range(9):
        cand = torch.cuda.current_stream(eng.dev) if n == 0 else torch.cuda.Stream(device=eng.dev)
        ok = _overlaps(torch, cand, eng.copy_stream) and _overlaps(torch, eng.copy_stream, cand)
        tried.append(ok)
        if ok:
            print(f"compute stream: candidate {n} runs beside the copy stream (tried: {tried})")
            return cand
    raise AssertionError(f"no stream runs beside the engine's copy stream: the held-back variants cannot hold anything back ({tried})")


def run_manual(torch, eng, job_lists, hold, cycles):
    """acquire / fill / submit from this thread, a slot reacquired as soon as the next job needs one; before the first submit
    of each pass a device-side sleep on the compute stream (hold="compute": uploads run ahead as far as the ring allows) or on
    the copy stream (hold="copy": compute is ready before the bytes arrive, and the producer side waits for its slots)"""
    taken, fill = _Taken(), make_fill()
    enqueue = []
    compute = compute_stream_beside(torch, eng)
    with torch.cuda.stream(compute):
        for jobs in job_lists:
            with torch.cuda.stream(eng.copy_stream if hold == "copy" else compute):
                torch.cuda._sleep(cycles)
            t0 = time.perf_counter()
            for key, loc in jobs:
                plan = eng.plan(*key)
                slot = eng.acquire()
                sizes, idx, imgs = slot.views(plan.b, plan.hp, plan.wp)
                sizes[0, :], sizes[1, :], idx[:] = plan.hp, plan.wp, 0      # tail entries as BatchFeeder writes them
                for j, i in enumerate(loc):
                    fill(i, j, sizes, idx, imgs)
                eng.submit(slot, plan, recycle=True)
                taken(plan, loc)
            enqueue.append(time.perf_counter() - t0)
    eng.sync()
    print(f"hold={hold}: host time per pass " + ", ".join(f"{1e3 * t:.2f} ms" for t in enqueue))
    return taken


def compare(taken, want, rules="cpp", times_each=2, canvases=None):
    """every submitted image: maps bit-equal to the image alone, record equal in all it defines; tail entries: a clean status"""
    from posepaf._lib import ST_DEFINED_MASK
    from posepaf.api import records_to_numpy
    seen = np.zeros(ec.N_IMAGES, np.int64)
    for n_job, (key, loc, maps, recs, canvas) in enumerate(taken.jobs):
        maps, recs = maps.cpu().numpy(), records_to_numpy(recs)
        canvas = canvas.cpu().numpy() if canvas is not None else None
        assert maps.shape[0] == key[2] == len(recs) and len(loc) <= key[2]
        for j, i in enumerate(loc):
            ctx = f"job {n_job} {key} entry {j}: image {i}"
            assert maps[j].shape == want["maps"][i].shape, ctx
            diff = int((_bits(maps[j]) != _bits(want["maps"][i])).sum())
            assert diff == 0, f"{ctx}: {diff} map elements differ from the image alone"
            assert _same_record(recs[j], want[rules][i]), \
                f"{ctx}: record differs (humans {int(recs[j]['n_humans'])} vs {int(want[rules][i]['n_humans'])})"
            if canvases is not None:
                h, w = ec.shapes()[i]
                assert np.array_equal(canvas[j, :h, :w], canvases(i)), f"{ctx}: canvas"
            seen[i] += 1
        for j in range(len(loc), key[2]):
            assert int(recs[j]["status"]) & ~ST_DEFINED_MASK == 0, (n_job, key, j)
    if times_each is not None:
        assert (seen == times_each).all(), seen.tolist()


def compare_scatter(out, want, rules):
    from posepaf.api import records_to_numpy
    recs = records_to_numpy(out.view(-1))
    for i in range(ec.N_IMAGES):
        assert _same_record(recs[i], want[rules][i]), f"row {i} of the scattered records"


# ------------------------------------------------------------------------------------------------ the variants
@pytest.mark.parametrize("use_graph", (True, False), ids=("graph", "eager"))
@pytest.mark.parametrize("rules", ("cpp", "py"))
def test_product_loop(torch_cuda, model, post, banks, truth, rules, use_graph):
    """a. engine.run_jobs with BatchFeeder(depth=2, workers=4): both passes, all 66 images twice, and the scattered rows"""
    eng = make_engine(torch_cuda, model, post, banks, rules=rules, use_graph=use_graph)
    taken, out = run_product_loop(torch_cuda, eng, ec.passes())
    assert len(taken.jobs) == 12
    compare(taken, truth, rules)
    compare_scatter(out, truth, rules)


def test_compute_held_back(torch_cuda, model, post, banks, truth):
    """b. the compute stream sleeps while the host enqueues a pass: every upload the ring admits is in flight before the first
    replay, and what keeps a staging buffer from being overwritten is the `consumed` event alone.
    Sleep: 25 million cycles = 10.4 ms per pass, four times the 2.6 ms the host was measured to need for a pass (see
    SLEEP_CYCLES).  On a scratch engine (b = 16 jobs of bucket A alone) this variant fails when submit() loses
    `self.copy_stream.wait_event(self.consumed[k])` (job 0 comes out with the pixels of job 2: 102388 map elements differ), and
    also when acquire() loses wait_host_writable(); it only does so on a compute stream that compute_stream_beside() has seen
    overlap the copy stream -- on the default stream the two shared a hardware queue in most engines and nothing ran ahead."""
    eng = make_engine(torch_cuda, model, post, banks)
    compare(run_manual(torch_cuda, eng, ec.passes(), "compute", SLEEP_CYCLES), truth)


def test_copy_stream_held_back(torch_cuda, model, post, banks, truth):
    """c. the copy stream sleeps: compute is enqueued before the bytes have landed (the upload event is what it waits for), and
    the thread that fills the slots gets a slot back only through wait_host_writable.
    Sleep: as in b, 25 million cycles = 10.4 ms per pass against 2.6 ms measured.  On a scratch engine (b = 16 jobs of bucket A
    alone, every staging buffer holding a valid header from an earlier pass) this variant fails when submit() loses
    `cur.wait_event(ev)` and when acquire() loses wait_host_writable() (job 0 differs in 102388 / 102394 map elements)."""
    eng = make_engine(torch_cuda, model, post, banks)
    compare(run_manual(torch_cuda, eng, ec.passes(), "copy", SLEEP_CYCLES), truth)


def test_device_scenes(torch_cuda, model, post, banks, truth_device):
    """d. scenes="device": joints, people counts and scene ids travel in the poisoned slot; non-zero noise keyed by the id"""
    eng = make_engine(torch_cuda, model, post, banks, scenes="device", max_people=ec.DEVICE_MAX_PEOPLE,
                      scene_noise=ec.DEVICE_NOISE, scene_seed=ec.DEVICE_SEED)
    taken, out = run_product_loop(torch_cuda, eng, ec.passes(), device_scenes=True)
    compare(taken, truth_device)
    compare_scatter(out, truth_device, "cpp")


def test_render(torch_cuda, model, post, banks, truth):
    """e. render=True: each job's canvas corner is the NumPy drawing of the image's own record on the image's own pixels"""
    from posepaf.render import draw_record_numpy
    drawn = {}

    def canvases(i):
        if i not in drawn:
            drawn[i] = draw_record_numpy(ec.image(i), truth["cpp"][i])
        return drawn[i]
    eng = make_engine(torch_cuda, model, post, banks, render=True)
    taken, out = run_product_loop(torch_cuda, eng, ec.passes(), render=True)
    compare(taken, truth, canvases=canvases)
    compare_scatter(out, truth, "cpp")
