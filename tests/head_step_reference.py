"""The loss-scale state machine of pp_head_update_f32 (include/posepaf.h: pp_head_update_state) restated in NumPy -- apex's dynamic
scaler: halve on a step whose gradient is not finite (the step is skipped), double after growth_interval finite steps in a row,
between min_scale and max_scale; growth_interval = 0 is a static scale.  Pure NumPy; nothing here imports the package.
tests/test_head_step_reference_cpu.py holds it against a table written out by hand."""
import numpy as np

FIELDS = ("scale", "inv_scale", "good_steps", "growth_interval", "min_scale", "max_scale", "skipped")
MIN_SCALE, MAX_SCALE = 2.0 ** -24, 2.0 ** 24


def new_state(scale, growth_interval, min_scale=MIN_SCALE, max_scale=MAX_SCALE, skipped=0):
    f = np.float32
    return dict(scale=f(scale), inv_scale=f(1.0) / f(scale), good_steps=0, growth_interval=int(growth_interval), min_scale=f(min_scale),
                max_scale=f(max_scale), skipped=int(skipped))


def advance(state, finite):
    """the state after one step whose gradients were all finite (True) or not (False) -> a new dict"""
    s = dict(state)
    if not finite:
        s["skipped"] += 1
    if s["growth_interval"] > 0:
        if not finite:
            s["scale"] = max(np.float32(s["scale"] * np.float32(0.5)), s["min_scale"])
            s["good_steps"] = 0
        else:
            s["good_steps"] += 1
            if s["good_steps"] >= s["growth_interval"]:
                s["scale"] = min(np.float32(s["scale"] * np.float32(2.0)), s["max_scale"])
                s["good_steps"] = 0
        s["inv_scale"] = np.float32(1.0) / s["scale"]
    return s


def run(state, outcomes):
    """-> the states after each of `outcomes` (True: finite)"""
    out = []
    for finite in outcomes:
        state = advance(state, finite)
        out.append(state)
    return out


def as_tuple(state):
    return tuple(float(state[k]) if isinstance(state[k], np.floating) else state[k] for k in FIELDS)
