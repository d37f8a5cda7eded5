#!/usr/bin/env python3
"""The binary16 fused residual tail (shl_mi355x_conv_add_f16_forward) against the launches it replaces, through the C-ABI (no
torch): tools/residual_bench.py for binary16 NHWC.

    python tools/residual_f16_bench.py [--reps 4] [--batches 1,128] [--only NAME[,NAME]] [--out FILE.md]
Per shape two hipGraphs are captured, each holding `reps` units of work that rotate over three buffer sets (so that a unit
does not find its operands in the last-level cache):
  * unfused   what a session captures with SHL_MI355X_RESIDUAL=0: shl_mi355x_conv_forward (the convolution in the family its
              own rules pick), shl_mi355x_add, shl_mi355x_relu_f16 (none for a MobileNetV2 projection, whose sum is the
              block's output);
  * fused     one launch per unit: what a session's STEP_CONV_ADD enqueues, in the family the size rule picks
              (SHL_MI355X_RESIDUAL_FORM forces the other one for an A/B run).
The two graphs are timed ALTERNATELY: five rounds, in each a window of replays of the unfused graph (as many as fill ~10 ms, at
least 20), then one of as many of the fused graph, between two HIP events.  The figure is the median of the five windows per unit, "spread" the range of the five windows
over their median.  Before timing, the fused output is compared with the unfused one on bits; the column "halves apart" counts
the differences.  Where the stand-alone convolution runs another family than the fused launch (row-patch, ping-pong, producer /
consumer, the wave kernel's split-K form against a tile kernel) its fp32 sums are rounded in another order and a few halves
differ by one unit in the last place of the convolution's value, as they do between those families without any tail; more
than that stops the run.  Prints a markdown table.

Shapes: ResNet-50 expansions (64 -> 256 @56, 128 -> 512 @28, 256 -> 1024 @14, 512 -> 2048 @7), ResNet-18/34 3x3 tails (64 @56,
128 @28, 256 @14, 512 @7), MobileNetV2 projections (144 -> 24 @56, 192 -> 32 @28, 384 -> 64 @14, 576 -> 96 @14, 960 -> 160 @7).
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
    # name, map, C, Co, kernel, activation behind the sum (0 none, 1 relu)
    ("r50_64_256_56", 56, 64, 256, 1, 1),
    ("r50_128_512_28", 28, 128, 512, 1, 1),
    ("r50_256_1024_14", 14, 256, 1024, 1, 1),
    ("r50_512_2048_7", 7, 512, 2048, 1, 1),
    ("r18_64_56_3x3", 56, 64, 64, 3, 1),
    ("r18_128_28_3x3", 28, 128, 128, 3, 1),
    ("r18_256_14_3x3", 14, 256, 256, 3, 1),
    ("r18_512_7_3x3", 7, 512, 512, 3, 1),
    ("mbv2_144_24_56", 56, 144, 24, 1, 0),
    ("mbv2_192_32_28", 28, 192, 32, 1, 0),
    ("mbv2_384_64_14", 14, 384, 64, 1, 0),
    ("mbv2_576_96_14", 14, 576, 96, 1, 0),
    ("mbv2_960_160_7", 7, 960, 160, 1, 0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--batches", default="1,128")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cases
    import residual_f16_cases as rc
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("residual_f16_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
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
            raise SystemExit("residual_f16_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
        hip.shl_mi355x_graph_launch(g, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "first replay")
        return g

    def window(g, replays):
        hip.shl_mi355x_event_record(ev0, stream)
        for _ in range(replays):
            hip.shl_mi355x_graph_launch(g, stream)
        hip.shl_mi355x_event_record(ev1, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "timed window")
        hip.shl_mi355x_event_elapsed_ms(ev0, ev1, C.byref(ms))
        return ms.value

    def figure(windows, units):
        windows = sorted(windows)
        return windows[2] * 1e-3 / units, (windows[-1] - windows[0]) / windows[2]

    head = ["shape", "M x Co x K bytes", "unfused kernels", "launches", "unfused us", "spread", "fused kernel", "fused us", "spread",
            "fused / unfused", "beyond the spread", "halves apart", "by default"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    only = set(filter(None, a.only.split(",")))
    for n in [int(b) for b in a.batches.split(",")]:
        for base, hw, c, co, k, act in SHAPES:
            name = "%s_b%d" % (base, n)
            if only and name not in only and base not in only:
                continue
            # (one image's worth of random data, repeated over the batch: the kernels do not look at values)
            cv = cases.make_case(9377, dtype="f16", n=1, h=hw, w=hw, c=c, co=co, k=(k, k), pad=(k // 2,) * 4)
            cv["input"] = np.ascontiguousarray(np.broadcast_to(cv["input"], (n,) + cv["input"].shape[1:]))
            cv["n"], cv["in_shape"], cv["out_shape"] = n, cv["input"].shape, (n,) + tuple(cv["out_shape"][1:])
            skip1 = (3 * np.random.default_rng(9477).standard_normal((1,) + tuple(cv["out_shape"][1:]))).astype(np.float16)
            case = dict(name=name, conv=cv, conv_first=1, act=act, skip=np.ascontiguousarray(np.broadcast_to(skip1, cv["out_shape"])))
            count = int(np.prod(cv["out_shape"]))
            plan = rc.make_plan(hip, cv)
            desc = rc.residual_desc(case)
            bufs = []
            for _ in range(SETS):
                b = dict(x=dev.alloc(cv["input"].nbytes), skip=dev.alloc(2 * count), conv=dev.alloc(2 * count), sum=dev.alloc(2 * count),
                         un=dev.alloc(2 * count), fused=dev.alloc(2 * count))
                dev.upload(b["x"], cv["input"])
                dev.upload(b["skip"], case["skip"])
                bufs.append(b)

            def unfused(kk):
                b = bufs[kk % SETS]
                pkg.check(hip.shl_mi355x_conv_forward(plan, b["x"], b["conv"], 0, stream), hip, "conv_forward")
                pkg.check(hip.shl_mi355x_add(b["conv"], b["skip"], b["sum"], count, pkg.SHL_F16, 1.0, 0, 1.0, 0, 1.0, 0, stream), hip, "add")
                if act:
                    pkg.check(hip.shl_mi355x_relu_f16(b["sum"], b["un"], count, 0, stream), hip, "relu_f16")

            def fused(kk):
                b = bufs[kk % SETS]
                pkg.check(hip.shl_mi355x_conv_add_f16_forward(plan, b["x"], b["skip"], b["fused"], 0, C.byref(desc), stream), hip,
                          "conv_add_f16_forward")

            def fetch(p):
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                return dev.download(p, (count,), np.float16)
            unfused(0)
            want, conv = fetch(bufs[0]["un" if act else "sum"]), fetch(bufs[0]["conv"])
            fused(0)
            flavour = hip.shl_mi355x_last_igemm_flavour().decode()
            got = fetch(bufs[0]["fused"])
            apart = int((got.view(np.uint16) != want.view(np.uint16)).sum())
            # one unit in the last place of the largest convolution value, carried through the 1-Lipschitz tail, and rare
            ulp = 2.0 ** -10 * float(np.abs(conv.astype(np.float32)).max())
            worst = float(np.abs(got.astype(np.float32) - want.astype(np.float32)).max())
            if worst > 2 * ulp or apart > count // 100:
                raise SystemExit("residual_f16_bench: %s: the fused launch differs from the unfused launches on %d halves, by up to %g"
                                 % (name, apart, worst))
            del want, conv, got
            g_un, g_f = capture(unfused, a.reps), capture(fused, a.reps)
            # windows of at least ~10 ms of the unfused graph (20 replays of a batch-1 shape are under a millisecond: the
            # clock's and the scheduler's noise, not the kernels')
            replays = int(min(2000, max(20, 20 * 10.0 / max(window(g_un, 20), 1e-3))))
            w_un, w_f = [], []
            for _ in range(5):
                w_un.append(window(g_un, replays))
                w_f.append(window(g_f, replays))
            hip.shl_mi355x_graph_destroy(g_un)
            hip.shl_mi355x_graph_destroy(g_f)
            (t_un, sp_un), (t_f, sp_f) = figure(w_un, replays * a.reps), figure(w_f, replays * a.reps)
            kbytes = (k * k * c * 2 + 63) // 64 * 64
            cells = [name, "%d x %d x %d" % (n * cv["ho"] * cv["wo"], co, kbytes),
                     hip.shl_mi355x_conv_plan_kernel_name(plan).decode().replace("conv_", "").replace("_f16_mfma32x32x16", "") +
                     (" + add + relu" if act else " + add"),
                     "1 / %d" % (3 if act else 2), "%.2f" % (t_un * 1e6), "%.0f %%" % (100 * sp_un), flavour, "%.2f" % (t_f * 1e6),
                     "%.0f %%" % (100 * sp_f), "%.2f" % (t_f / t_un), "yes" if t_f / t_un < 1.0 - sp_un else "no", str(apart),
                     "yes" if hip.shl_mi355x_conv_add_f16_by_default(plan, 0) else "no"]
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
