#!/usr/bin/env python3
"""Depthwise Kh x Kw on the matrix cores (csrc/dwconv_kxk.hip) against the generic kernel it replaces, through the C-ABI (no torch).

    python tools/dw_kxk_bench.py [--reps 4] [--only NAME[,NAME]] [--out FILE.md]
SHL_MI355X_DWKXK is read once per process, so the two sides are two worker processes of this script on the same build: one
under =1 (dwconv_kxk_mfma_i8 wherever the geometry fits), one under =0 (exactly the parent commit's code path, the baseline).
Per shape each worker captures one hipGraph holding `reps` shl_mi355x_conv_forward calls that rotate over three buffer sets (so
that a call does not find its operands in the last-level cache).  The parent times them ALTERNATELY: five rounds, in each a
window of replays of the generic graph, then one of the new kernel's, between two HIP events; a window is sized to ~50 ms from
a first untimed one.  The figure is the median of the five windows per call, "spread" the range of the five windows over their
median.  Before timing, the CRCs of the two outputs are compared.  Prints a markdown table; "wins" says whether the new kernel
was faster by more than the larger of the two spreads, the criterion of csrc/lut_validate.h.

Shapes: the 5x5 depthwise layers of MobileNetV3-Large and EfficientNet-B0 at batch 1 and 32 (those of tools/dw_act_bench.py),
and ConvNeXt-T's 7x7 layers at batch 1 and 8.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = 3
NETS = [
    # name, input map, C, kernel, stride, batches
    ("mbv3_5x5s2_672_14", 14, 672, 5, 2, (1, 32)),
    ("mbv3_5x5_960_7", 7, 960, 5, 1, (1, 32)),
    ("effnet_5x5s2_144_56", 56, 144, 5, 2, (1, 32)),
    ("effnet_5x5_240_28", 28, 240, 5, 1, (1, 32)),
    ("effnet_5x5_480_14", 14, 480, 5, 1, (1, 32)),
    ("effnet_5x5_672_14", 14, 672, 5, 1, (1, 32)),
    ("effnet_5x5_1152_7", 7, 1152, 5, 1, (1, 32)),
    ("convnext_7x7_96_56", 56, 96, 7, 1, (1, 8)),
    ("convnext_7x7_192_28", 28, 192, 7, 1, (1, 8)),
    ("convnext_7x7_384_14", 14, 384, 7, 1, (1, 8)),
    ("convnext_7x7_768_7", 7, 768, 7, 1, (1, 8)),
]
SHAPES = [(name + "_b%d" % n, n, hw, c, k, s) for (name, hw, c, k, s, batches) in NETS for n in batches]


def worker(a, shapes):
    """one side: per shape `ready <kernel> <crc>`, then a window of N replays per `w N` line (its milliseconds back), `n`: next"""
    import cases
    import residual_cases as rc
    pkg = cases.pkg
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("dw_kxk_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()
    for name, n, hw, c, k, stride in shapes:
        cv = cases.make_case(9779, n=n, h=hw, w=hw, c=c, depthwise=True, k=(k, k), stride=(stride, stride), pad=(k // 2,) * 4, exact=False)
        count = int(np.prod(cv["out_shape"]))
        plan = rc.make_plan(hip, cv)
        bufs = []
        for _ in range(SETS):
            b = dict(x=dev.alloc(cv["input"].nbytes), y=dev.alloc(count))
            dev.upload(b["x"], cv["input"])
            bufs.append(b)

        def enqueue(kk):
            b = bufs[kk % SETS]
            pkg.check(hip.shl_mi355x_conv_forward(plan, b["x"], b["y"], 0, stream), hip, "conv_forward")
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        crc = zlib.crc32(dev.download(bufs[0]["y"], (count,), np.int8).tobytes())
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for kk in range(a.reps):
            enqueue(kk)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("dw_kxk_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
        hip.shl_mi355x_graph_launch(g, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "first replay")
        print("ready", hip.shl_mi355x_conv_plan_kernel_name(plan).decode(), crc, flush=True)
        while True:
            line = sys.stdin.readline()
            if not line:
                raise SystemExit("dw_kxk_bench: the parent went away")  # (the other side failed: nothing more is launched)
            if line.startswith("n"):
                break
            hip.shl_mi355x_event_record(ev0, stream)
            for _ in range(int(line.split()[1])):
                hip.shl_mi355x_graph_launch(g, stream)
            hip.shl_mi355x_event_record(ev1, stream)
            pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "timed window")
            hip.shl_mi355x_event_elapsed_ms(ev0, ev1, C.byref(ms))
            print("%.6f" % ms.value, flush=True)
        hip.shl_mi355x_graph_destroy(g)
        for b in bufs:
            for p in b.values():
                dev.free(p)
        hip.shl_mi355x_conv_plan_destroy(plan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    shapes = [s for s in SHAPES if not only or s[0] in only]
    if a.worker:
        return worker(a, shapes)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps), "--only", a.only]
    sides = [subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=dict(os.environ, SHL_MI355X_DWKXK=v))
             for v in ("0", "1")]

    def ask(p, text=None):
        if text is not None:
            p.stdin.write(text + "\n")
            p.stdin.flush()
        line = p.stdout.readline()
        if not line:
            for q in sides:
                if q is not p:
                    q.kill()
            raise SystemExit("dw_kxk_bench: a worker ended early (exit %s)" % p.wait())
        return line.split()

    def figure(windows, calls):
        windows = sorted(windows)
        return windows[2] * 1e-3 / calls, (windows[-1] - windows[0]) / windows[2]

    head = ["shape", "M x C x taps", "generic us", "spread", "kernel at =1", "new us", "spread", "new / generic", "wins"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for name, n, hw, c, k, stride in shapes:
        ho = (hw + 2 * (k // 2) - k) // stride + 1
        dims = "%d x %d x %d" % (n * ho * ho, c, k * k)
        ready = [ask(p) for p in sides]
        if ready[0][1] != "dwconv_nhwc_i8" or ready[0][2] != ready[1][2]:
            raise SystemExit("dw_kxk_bench: %s: baseline kernel %s, CRCs %s / %s" % (name, ready[0][1], ready[0][2], ready[1][2]))
        replays = []
        for p in sides:  # an untimed window sizes the timed ones to ~50 ms
            t20 = float(ask(p, "w 20")[0])
            replays.append(max(20, min(4000, int(20 * 50.0 / max(t20, 1e-3)))))
        w = ([], [])
        for _ in range(5):
            for i, p in enumerate(sides):
                w[i].append(float(ask(p, "w %d" % replays[i])[0]))
        for p in sides:
            p.stdin.write("n\n")
            p.stdin.flush()
        (t0, sp0), (t1, sp1) = figure(w[0], replays[0] * a.reps), figure(w[1], replays[1] * a.reps)
        wins = t1 / t0 < 1.0 - max(sp0, sp1)
        cells = [name, dims, "%.2f" % (t0 * 1e6), "%.0f %%" % (100 * sp0), ready[1][1], "%.2f" % (t1 * 1e6), "%.0f %%" % (100 * sp1),
                 "%.2f" % (t1 / t0), "-" if ready[1][1] == ready[0][1] else "yes" if wins else "no"]  # (-: outside the kernel's scope)
        row = "| " + " | ".join(cells) + " |"
        lines.append(row)
        print(row, flush=True)
    for p in sides:
        p.stdin.close()
        if p.wait() != 0:
            raise SystemExit("dw_kxk_bench: a worker failed (exit %d)" % p.returncode)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
