#!/usr/bin/env python3
"""A table activation in the depthwise launch (shl_mi355x_dwconv_lut_forward) against the two launches it replaces, through the
C-ABI (no torch).

    python tools/dw_act_bench.py [--reps 4] [--only NAME[,NAME]] [--out FILE.md]
Per shape two hipGraphs are captured, each holding `reps` units of work that rotate over three buffer sets (so that a unit
does not find its operands in the last-level cache):
  * unfused   what a session captures with SHL_MI355X_ACT_FUSE=0, the parent commit's code path: shl_mi355x_conv_forward, then
              shl_mi355x_unary_lut_i8;
  * fused     one launch per unit: what a session's STEP_CONV_LUT enqueues on a depthwise plan, on the kernel conv_forward runs
              for the same plan and batch (SHL_MI355X_DWMFMA=0|1 moves both sides for an A/B run).
The two graphs are timed ALTERNATELY: five rounds, in each a window of 20 replays of the unfused graph, then one of the fused
graph, between two HIP events.  The figure is the median of the five windows per unit, "spread" the range of the five windows
over their median.  Before timing, the fused output is compared with the unfused one byte for byte.  Prints a markdown table;
"wins" says whether fused was faster by more than the larger of the two spreads, the criterion of csrc/lut_validate.h.

Shapes: the depthwise layers in front of a hard-swish in MobileNetV3-Large and in front of a swish in EfficientNet-B0, at batch 1
and at batch 32.
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
NETS = [
    # name, input map, C, kernel, stride
    ("mbv3_3x3s2_240_28", 28, 240, 3, 2),   # (EfficientNet-B0 has the same layer)
    ("mbv3_3x3_200_14", 14, 200, 3, 1),
    ("mbv3_3x3_184_14", 14, 184, 3, 1),
    ("mbv3_3x3_480_14", 14, 480, 3, 1),
    ("mbv3_3x3_672_14", 14, 672, 3, 1),
    ("effnet_3x3_32_112", 112, 32, 3, 1),
    ("effnet_3x3_144_56", 56, 144, 3, 1),
    ("effnet_3x3_1152_7", 7, 1152, 3, 1),
    ("mbv3_5x5s2_672_14", 14, 672, 5, 2),
    ("mbv3_5x5_960_7", 7, 960, 5, 1),
    ("effnet_5x5s2_144_56", 56, 144, 5, 2),
    ("effnet_5x5_240_28", 28, 240, 5, 1),
    ("effnet_5x5_480_14", 14, 480, 5, 1),
    ("effnet_5x5_672_14", 14, 672, 5, 1),
    ("effnet_5x5_1152_7", 7, 1152, 5, 1),
]
SHAPES = [(name + "_b%d" % n, n) + tuple(rest) for n in (1, 32) for (name, *rest) in NETS]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cases
    import residual_cases as rc
    pkg = cases.pkg
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("dw_act_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()

    def capture(enqueue, reps):
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for k in range(reps):
            enqueue(k)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("dw_act_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
        hip.shl_mi355x_graph_launch(g, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "first replay")
        return g

    def window(g):
        hip.shl_mi355x_event_record(ev0, stream)
        for _ in range(20):
            hip.shl_mi355x_graph_launch(g, stream)
        hip.shl_mi355x_event_record(ev1, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "timed window")
        hip.shl_mi355x_event_elapsed_ms(ev0, ev1, C.byref(ms))
        return ms.value

    def figure(windows, reps):
        windows = sorted(windows)
        return windows[2] * 1e-3 / (20 * reps), (windows[-1] - windows[0]) / windows[2]

    head = ["shape", "M x C x taps", "unfused us", "spread", "fused kernel", "fused us", "spread", "fused / unfused", "wins", "by default"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    only = set(filter(None, a.only.split(",")))
    for name, n, hw, c, k, stride in SHAPES:
        if only and name not in only:
            continue
        cv = cases.make_case(9778, n=n, h=hw, w=hw, c=c, depthwise=True, k=(k, k), stride=(stride, stride), pad=(k // 2,) * 4, exact=False)
        count = int(np.prod(cv["out_shape"]))
        dims = "%d x %d x %d" % (n * cv["ho"] * cv["wo"], c, k * k)
        plan = rc.make_plan(hip, cv)
        if not hip.shl_mi355x_dwconv_lut_fusable(plan, 0):
            row = "| " + " | ".join([name, dims, "-", "-", "none: the plan is not one the fused launch takes", "-", "-", "-", "-", "no"]) + " |"
            lines.append(row)
            print(row, flush=True)
            hip.shl_mi355x_conv_plan_destroy(plan)
            continue
        table = np.zeros(256, np.uint8)
        opt.shl_mi355x_silu_table_i8(float(np.float32(cv["out_scale"])), cv["out_zp"], float(np.float32(0.0219)), 4,
                                     table.ctypes.data_as(C.POINTER(C.c_uint8)))
        bufs = []
        for _ in range(SETS):
            b = dict(x=dev.alloc(cv["input"].nbytes), conv=dev.alloc(count), un=dev.alloc(count), fused=dev.alloc(count))
            dev.upload(b["x"], cv["input"])
            bufs.append(b)

        def unfused(kk):
            b = bufs[kk % SETS]
            pkg.check(hip.shl_mi355x_conv_forward(plan, b["x"], b["conv"], 0, stream), hip, "conv_forward")
            pkg.check(hip.shl_mi355x_unary_lut_i8(b["conv"], b["un"], count, table.ctypes.data, stream), hip, "unary_lut_i8")

        def fused(kk):
            b = bufs[kk % SETS]
            pkg.check(hip.shl_mi355x_dwconv_lut_forward(plan, b["x"], b["fused"], 0, table.ctypes.data, stream), hip, "dwconv_lut_forward")

        def fetch(p):
            pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
            return dev.download(p, (count,), np.int8)
        unfused(0)
        want = fetch(bufs[0]["un"])
        fused(0)
        if not np.array_equal(fetch(bufs[0]["fused"]), want):
            raise SystemExit("dw_act_bench: %s: the fused launch differs from the unfused launches" % name)
        g_un, g_f = capture(unfused, a.reps), capture(fused, a.reps)
        w_un, w_f = [], []
        for _ in range(5):
            w_un.append(window(g_un))
            w_f.append(window(g_f))
        hip.shl_mi355x_graph_destroy(g_un)
        hip.shl_mi355x_graph_destroy(g_f)
        (t_un, sp_un), (t_f, sp_f) = figure(w_un, a.reps), figure(w_f, a.reps)
        wins = t_f / t_un < 1.0 - max(sp_un, sp_f)
        cells = [name, dims, "%.2f" % (t_un * 1e6), "%.0f %%" % (100 * sp_un), hip.shl_mi355x_dwconv_lut_kernel_name(plan, 0).decode(),
                 "%.2f" % (t_f * 1e6), "%.0f %%" % (100 * sp_f), "%.2f" % (t_f / t_un), "yes" if wins else "no",
                 "yes" if hip.shl_mi355x_dwconv_lut_by_default(plan, 0) else "no"]
        row = "| " + " | ".join(cells) + " |"
        lines.append(row)
        print(row, flush=True)
        for b in bufs:
            for p in b.values():
                dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
