#!/usr/bin/env python3
"""Dense int8 layers whose channel count is no multiple of 16 on the matrix cores (csrc/conv_igemm_cpad.hip) against the direct kernel
they ran on, through the C-ABI (no torch).

    python tools/cpad_bench.py [--reps 4] [--only NAME[,NAME]] [--out FILE.md]
The two sides are two worker processes of this script on the same build: one under SHL_MI355X_CPAD=1
(conv_igemm_cpad_i8_mfma32x32x32 wherever the geometry fits), one under =0 (exactly the parent commit's code path, the baseline).
Per shape each worker captures one hipGraph holding `reps` shl_mi355x_conv_forward calls that rotate over three buffer sets (so that
a call does not find its operands in the last-level cache); for an NCHW layer a call of the new side is three launches -- the
NCHW -> NHWC re-layout, the kernel, the re-layout back -- and all three are in its time.  The parent times the graphs ALTERNATELY:
five rounds, in each a window of replays of the direct graph, then one of the new kernel's, between two HIP events; a window is
sized to ~50 ms from a first untimed one.  The figure is the median of the five windows per call, "spread" the range of the five
windows over their median.  Before timing, the CRCs of the two outputs are compared.  Prints a markdown table; "wins" says whether
the new kernel's median lies below the direct kernel's by more than the two spreads TOGETHER (cpad.h:cp_default's criterion).

Shapes: the pointwise layers of MobileNetV2 / V3 and ShuffleNetV2 1.0x with such widths and two 3x3 layers, at batch 1, 8 and 32;
NHWC for all, NCHW for the first of each model.
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
    # name, input map, Cin, Cout, k, NCHW too
    ("mbv2_24to144_56", 56, 24, 144, 1, True), ("mbv2_144to24_56", 56, 144, 24, 1, False),
    ("mbv3_72to24_56", 56, 72, 24, 1, True), ("mbv3_72to40_28", 28, 72, 40, 1, False), ("mbv3_40to120_28", 28, 40, 120, 1, False),
    ("mbv3_120to40_28", 28, 120, 40, 1, False), ("mbv3_200to80_14", 14, 200, 80, 1, False), ("mbv3_184to80_14", 14, 184, 80, 1, False),
    ("shuf_58to58_28", 28, 58, 58, 1, True), ("shuf_116to116_14", 14, 116, 116, 1, False), ("shuf_232to232_7", 7, 232, 232, 1, False),
    ("3x3_24to24_56", 56, 24, 24, 3, True), ("3x3_40to40_28", 28, 40, 40, 3, False),
]
SHAPES = [("%s_b%d_%s" % (name, n, lay.lower()), n, lay, hw, c, co, k) for (name, hw, c, co, k, nchw) in NETS for n in (1, 8, 32)
          for lay in (("NHWC", "NCHW") if nchw else ("NHWC",))]


def worker(a, shapes):
    """one side: per shape `ready <kernel> <crc>`, then a window of N replays per `w N` line (its milliseconds back), `n`: next"""
    import cases
    import residual_cases as rc
    pkg = cases.pkg
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("cpad_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()
    for name, n, lay, hw, c, co, k in shapes:
        cv = cases.make_case(9783, layout=lay, n=n, h=hw, w=hw, c=c, co=co, k=(k, k), pad=(k // 2,) * 4, exact=False, act=1)
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
            raise SystemExit("cpad_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
        hip.shl_mi355x_graph_launch(g, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "first replay")
        print("ready", hip.shl_mi355x_conv_plan_kernel_name(plan).decode(), crc, flush=True)
        while True:
            line = sys.stdin.readline()
            if not line:
                raise SystemExit("cpad_bench: the parent went away")  # (the other side failed: nothing more is launched)
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
    sides = [subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=dict(os.environ, SHL_MI355X_CPAD=v))
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
            raise SystemExit("cpad_bench: a worker ended early (exit %s)" % p.wait())
        return line.split()

    def figure(windows, calls):
        windows = sorted(windows)
        return windows[2] * 1e-3 / calls, (windows[-1] - windows[0]) / windows[2]

    head = ["shape", "M x Cout x K", "direct us", "spread", "kernel at =1", "new us", "spread", "new / direct", "wins"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for name, n, lay, hw, c, co, k in shapes:
        dims = "%d x %d x %d" % (n * hw * hw, co, k * k * c)
        ready = [ask(p) for p in sides]
        if ready[0][1] == ready[1][1]:  # outside the kernel's scope (144 channels are nine whole chunks: the implicit GEMM's layer)
            for p in sides:
                p.stdin.write("n\n")
                p.stdin.flush()
            lines.append("| " + " | ".join([name, dims, "-", "-", ready[1][1], "-", "-", "-", "-"]) + " |")
            print(lines[-1], flush=True)
            continue
        if "direct" not in ready[0][1] or ready[0][2] != ready[1][2]:
            raise SystemExit("cpad_bench: %s: baseline kernel %s, checksums %s / %s" % (name, ready[0][1], ready[0][2], ready[1][2]))
        replays = []
        for p in sides:  # an untimed window sizes the timed ones to ~50 ms
            t5 = float(ask(p, "w 5")[0])
            replays.append(max(5, min(4000, int(5 * 50.0 / max(t5, 1e-3)))))
        w = ([], [])
        for _ in range(5):
            for i, p in enumerate(sides):
                w[i].append(float(ask(p, "w %d" % replays[i])[0]))
        for p in sides:
            p.stdin.write("n\n")
            p.stdin.flush()
        (t0, sp0), (t1, sp1) = figure(w[0], replays[0] * a.reps), figure(w[1], replays[1] * a.reps)
        wins = t1 / t0 < 1.0 - (sp0 + sp1)
        cells = [name, dims, "%.2f" % (t0 * 1e6), "%.0f %%" % (100 * sp0), ready[1][1], "%.2f" % (t1 * 1e6), "%.0f %%" % (100 * sp1),
                 "%.2f" % (t1 / t0), "yes" if wins else "no"]
        row = "| " + " | ".join(cells) + " |"
        lines.append(row)
        print(row, flush=True)
    for p in sides:
        p.stdin.close()
        if p.wait() != 0:
            raise SystemExit("cpad_bench: a worker failed (exit %d)" % p.returncode)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
