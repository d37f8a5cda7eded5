#!/usr/bin/env python3
"""The fused residual tail (shl_mi355x_conv_add_forward) against the launches it replaces, through the C-ABI (no torch).

    python tools/residual_bench.py [--reps 4] [--only NAME[,NAME]] [--out FILE.md]
Per shape two hipGraphs are captured, each holding `reps` units of work that rotate over three buffer sets (so that a unit
does not find its operands in the last-level cache):
  * unfused   what a session captures with SHL_MI355X_RESIDUAL=0, the parent commit's kernels: shl_mi355x_conv_forward (the
              convolution in the family its own rules pick), shl_mi355x_add, shl_mi355x_relu_i8 (none for a MobileNetV2
              projection, whose sum is the block's output);
  * fused     one launch per unit: what a session's STEP_CONV_ADD enqueues, in the family the size rule picks
              (SHL_MI355X_RESIDUAL_FORM forces the other one for an A/B run).
The two graphs are timed ALTERNATELY: five rounds, in each a window of 20 replays of the unfused graph, then one of the fused
graph, between two HIP events.  The figure is the median of the five windows per unit, "spread" the range of the five windows
over their median.  Before timing, the fused output is compared with the unfused one byte for byte.  Prints a markdown table.

Shapes: ResNet-50 bottleneck tails (the 1x1 expansion in front of the add: 256 -> 1024 @14, 512 -> 2048 @7, 64 -> 256 @56) at
batch 1 and 128, ResNet-18's 3x3 tails (64 @56, 512 @7) at batch 1 and 128, MobileNetV2's projections at batch 1 (144 -> 24 @56,
192 -> 32 @28, 384 -> 64 @14, 960 -> 160 @7).
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
SHAPES = [
    # name, batch, map, C, Co, kernel, activation behind the sum (0 none, 1 relu)
    ("r50_256_1024_14_b1", 1, 14, 256, 1024, 1, 1),
    ("r50_512_2048_7_b1", 1, 7, 512, 2048, 1, 1),
    ("r50_64_256_56_b1", 1, 56, 64, 256, 1, 1),
    ("r18_64_56_3x3_b1", 1, 56, 64, 64, 3, 1),
    ("r18_512_7_3x3_b1", 1, 7, 512, 512, 3, 1),
    ("mbv2_144_24_56_b1", 1, 56, 144, 24, 1, 0),
    ("mbv2_192_32_28_b1", 1, 28, 192, 32, 1, 0),
    ("mbv2_384_64_14_b1", 1, 14, 384, 64, 1, 0),
    ("mbv2_960_160_7_b1", 1, 7, 960, 160, 1, 0),
    ("r50_256_1024_14_b128", 128, 14, 256, 1024, 1, 1),
    ("r50_512_2048_7_b128", 128, 7, 512, 2048, 1, 1),
    ("r50_64_256_56_b128", 128, 56, 64, 256, 1, 1),
    ("r18_64_56_3x3_b128", 128, 56, 64, 64, 3, 1),
    ("r18_512_7_3x3_b128", 128, 7, 512, 512, 3, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cases
    import residual_cases as rc
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("residual_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
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
            raise SystemExit("residual_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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

    head = ["shape", "M x Co x K bytes", "unfused kernels", "launches", "unfused us", "spread", "fused kernel", "fused us", "spread",
            "fused / unfused", "by default"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    only = set(filter(None, a.only.split(",")))
    for name, n, hw, c, co, k, act in SHAPES:
        if only and name not in only:
            continue
        case = rc._case(name, "auto", dict(n=n, h=hw, w=hw, c=c, co=co, k=(k, k), pad=(k // 2,) * 4, exact=False), conv_first=1, act=act,
                        skip_q=(0.0437, 5), sum_q=(0.0713, -9), out_q=(0.0519, -128), seed=77)
        cv = case["conv"]
        count = int(np.prod(cv["out_shape"]))
        plan = rc.make_plan(hip, cv)
        desc = rc.residual_desc(case)
        bufs = []
        for _ in range(SETS):
            b = dict(x=dev.alloc(cv["input"].nbytes), skip=dev.alloc(count), conv=dev.alloc(count), sum=dev.alloc(count),
                     un=dev.alloc(count), fused=dev.alloc(count))
            dev.upload(b["x"], cv["input"])
            dev.upload(b["skip"], case["skip"])
            bufs.append(b)
        conv_q = (float(np.float32(cv["out_scale"])), cv["out_zp"])

        def unfused(kk):
            b = bufs[kk % SETS]
            pkg.check(hip.shl_mi355x_conv_forward(plan, b["x"], b["conv"], 0, stream), hip, "conv_forward")
            pkg.check(hip.shl_mi355x_add(b["conv"], b["skip"], b["sum"], count, pkg.SHL_I8, conv_q[0], conv_q[1], case["skip_q"][0],
                                         case["skip_q"][1], case["sum_q"][0], case["sum_q"][1], stream), hip, "add")
            if act:
                pkg.check(hip.shl_mi355x_relu_i8(b["sum"], b["un"], count, case["sum_q"][0], case["sum_q"][1], case["out_q"][0],
                                                 case["out_q"][1], 0, stream), hip, "relu_i8")

        def fused(kk):
            b = bufs[kk % SETS]
            pkg.check(hip.shl_mi355x_conv_add_forward(plan, b["x"], b["skip"], b["fused"], 0, C.byref(desc), stream), hip, "conv_add_forward")

        def fetch(p):
            pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
            return dev.download(p, (count,), np.int8)
        unfused(0)
        want = fetch(bufs[0]["un" if act else "sum"])
        fused(0)
        if not np.array_equal(fetch(bufs[0]["fused"]), want):
            raise SystemExit("residual_bench: %s: the fused launch differs from the unfused launches" % name)
        g_un, g_f = capture(unfused, a.reps), capture(fused, a.reps)
        w_un, w_f = [], []
        for _ in range(5):
            w_un.append(window(g_un))
            w_f.append(window(g_f))
        hip.shl_mi355x_graph_destroy(g_un)
        hip.shl_mi355x_graph_destroy(g_f)
        (t_un, sp_un), (t_f, sp_f) = figure(w_un, a.reps), figure(w_f, a.reps)
        kbytes = (k * k * c + 63) // 64 * 64
        cells = [name, "%d x %d x %d" % (n * cv["ho"] * cv["wo"], co, kbytes),
                 hip.shl_mi355x_conv_plan_kernel_name(plan).decode().replace("conv_", "").replace("_i8_mfma32x32x32", "") + (" + add + relu" if act else " + add"),
                 "1 / %d" % (3 if act else 2), "%.2f" % (t_un * 1e6), "%.0f %%" % (100 * sp_un),
                 hip.shl_mi355x_conv_add_kernel_name(plan, 0).decode(), "%.2f" % (t_f * 1e6), "%.0f %%" % (100 * sp_f), "%.2f" % (t_f / t_un),
                 "yes" if hip.shl_mi355x_conv_add_by_default(plan, 0) else "no"]
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
