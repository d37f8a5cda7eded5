#!/usr/bin/env python3
"""The two forms of the transposed convolution against each other and against a yardstick, through the C-ABI (no torch).

    python tools/deconv_bench.py [--batches 1,32] [--reps 12] [--out FILE.md]
Layers (int8 NHWC, and binary16 NHWC): 2x2 stride 2 at 256 -> 128 @28 and 128 -> 64 @56, 4x4 stride 2 pad 1 at 128 -> 64 @32,
each at every batch of --batches.  Per layer: the phase form (SHL_MI355X_DECONV_FORM=phase), the gather form (=gather) -- both
first compared on the device's own data -- and, for the 2x2 stride-2 layers, the project's pointwise plan of equal work: a
2x2 s2 deconvolution Cin -> Co on H x W is a 1x1 convolution Cin -> 4 Co on the same map, the same MACs and the same bytes in
and out.  Timing as tools/resize_bench.py: `reps` launches captured in one hipGraph rotating over three buffer sets, the
graph replayed 20 times between two HIP events, median of five such windows, their spread beside it.  Prints a markdown
table; the ratio to the pointwise plan is recorded, not gated.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = 3
LAYERS = [  # (kernel, stride, pad, Cin, Co, map)
    (2, 2, 0, 256, 128, 28),
    (2, 2, 0, 128, 64, 56),
    (4, 2, 1, 128, 64, 32),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cases
    import deconv_cases as dc
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("deconv_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()

    def timed(enqueue):
        """enqueue(k): the k-th launch on `stream`; (seconds per launch, spread of the windows as a fraction)"""
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for k in range(a.reps):
            enqueue(k)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("deconv_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
        hip.shl_mi355x_graph_launch(g, stream)
        hip.shl_mi355x_stream_sync(stream)
        windows = []
        for _ in range(5):
            hip.shl_mi355x_event_record(ev0, stream)
            for _ in range(20):
                hip.shl_mi355x_graph_launch(g, stream)
            hip.shl_mi355x_event_record(ev1, stream)
            pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "timed window")
            hip.shl_mi355x_event_elapsed_ms(ev0, ev1, C.byref(ms))
            windows.append(ms.value)
        hip.shl_mi355x_graph_destroy(g)
        windows.sort()
        return windows[2] * 1e-3 / (20 * a.reps), (windows[-1] - windows[0]) / windows[2]

    def plan_of(create, desc, case, mult, bias):
        plan = C.c_void_p()
        pkg.check(create(C.byref(desc), case["kernel"].ctypes.data, mult.ctypes.data if case["dtype"] == "int8" else None, bias.ctypes.data,
                         None, C.byref(plan)), hip, "plan_create")
        return plan

    lines = ["| layer | batch | dtype | phase kernel | phase us | gather us | gather / phase | 1x1 plan | 1x1 us | phase / 1x1 | TMAC/s | spread |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    os.environ["SHL_MI355X_TUNE"] = "0"  # the yardstick by the selection rules: the same kernel on every box
    for n in [int(v) for v in a.batches.split(",")]:
        for k, s, p, cin, co, hw in LAYERS:
            for dtype in ("int8", "f16"):
                case = dc.make("bench_%d_%d_%d_%s" % (k, cin, hw, dtype), dtype=dtype, regime="general", n=n, h=hw, w=hw, c=cin, co=co,
                               k=(k, k), stride=(s, s), pad=(p,) * 4, normal=True)
                es = 1 if dtype == "int8" else 2
                mult, bias = dc.tables(case)
                in_b, out_b = case["x"].nbytes, int(np.prod(case["out_shape"])) * es
                ins = [dev.alloc(in_b) for _ in range(SETS)]
                outs = [dev.alloc(out_b) for _ in range(SETS)]
                for b in ins:
                    dev.upload(b, case["x"])
                plans = {}
                for form in (dc.PHASE, dc.GATHER):
                    os.environ["SHL_MI355X_DECONV_FORM"] = form
                    plans[form] = plan_of(hip.shl_mi355x_deconv_plan_create, dc.deconv_desc(case), case, mult, bias)
                del os.environ["SHL_MI355X_DECONV_FORM"]
                name = hip.shl_mi355x_conv_plan_kernel_name(plans[dc.PHASE]).decode()

                def launcher(plan):
                    return lambda kk: pkg.check(hip.shl_mi355x_conv_forward(plan, ins[kk % SETS], outs[kk % SETS], n, stream), hip, "forward")
                # the same answer from both forms on this data (binary16: within the project's 1e-3)
                launcher(plans[dc.PHASE])(0)
                launcher(plans[dc.GATHER])(1)
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                np_dt = np.int8 if es == 1 else np.float16
                got, lit = dev.download(outs[0], case["out_shape"], np_dt), dev.download(outs[1], case["out_shape"], np_dt)
                if not dc.matches(got, lit, dtype):
                    raise SystemExit("deconv_bench: %dx%d s%d %d -> %d @%d %s: the forms differ" % (k, k, s, cin, co, hw, dtype))
                t_ph, sp_ph = timed(launcher(plans[dc.PHASE]))
                t_ga, sp_ga = timed(launcher(plans[dc.GATHER]))
                pw_name, t_pw = "-", None
                if k == 2 and s == 2 and p == 0:  # the pointwise plan of equal work: [4 Co, 1, 1, Cin] on the same map
                    pw = dict(case, kernel=np.ascontiguousarray(case["kernel"].transpose(1, 2, 0, 3).reshape(4 * co, 1, 1, cin)))
                    d = dc.deconv_desc(case, out_h=hw, out_w=hw, out_c=4 * co, kernel_h=1, kernel_w=1, stride_h=1, stride_w=1)
                    mult4, bias4 = np.ascontiguousarray(np.tile(mult, 4)), np.ascontiguousarray(np.tile(bias, 4))
                    plan_pw = plan_of(hip.shl_mi355x_conv_plan_create, d, pw, mult4, bias4)
                    pw_name = hip.shl_mi355x_conv_plan_kernel_name(plan_pw).decode()
                    t_pw, _ = timed(launcher(plan_pw))
                    hip.shl_mi355x_conv_plan_destroy(plan_pw)
                macs = n * hw * hw * cin * co * k * k
                lines.append("| %dx%d s%d %d -> %d @%d | %d | %s | %s | %.1f | %.1f | %.2f | %s | %s | %s | %.2f | %.0f %% / %.0f %% |" % (
                    k, k, s, cin, co, hw, n, dtype, name, t_ph * 1e6, t_ga * 1e6, t_ga / t_ph, pw_name,
                    "%.1f" % (t_pw * 1e6) if t_pw else "-", "%.2f" % (t_ph / t_pw) if t_pw else "-", macs / t_ph / 1e12, 100 * sp_ph, 100 * sp_ga))
                print(lines[-1], flush=True)
                for plan in plans.values():
                    hip.shl_mi355x_conv_plan_destroy(plan)
                for b in ins + outs:
                    dev.free(b)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
