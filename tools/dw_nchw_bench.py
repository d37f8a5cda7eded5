#!/usr/bin/env python3
"""Depthwise NCHW layers whose kernel is not 3x3 (csrc/dwconv_kxk_nchw.hip), int8 and binary16, against the direct kernel they ran
on, through the C-ABI (no torch).

    python tools/dw_nchw_bench.py [--reps 4] [--only NAME[,NAME]] [--out FILE.md]
The two sides are two worker processes of this script on the same build: one under SHL_MI355X_DWNCHW=1 (dwconv_kxk_nchw_i8 / _f16
wherever scope and geometry fit), one under =0 (exactly the parent commit's code path, the baseline).  Per shape each worker
captures one hipGraph holding `reps` shl_mi355x_conv_forward calls that rotate over three buffer sets (so that a call does not find
its operands in the last-level cache).  The parent times the graphs ALTERNATELY: five rounds, in each a window of replays of the
direct graph, then one of the new kernel's, between two HIP events; a window is sized to ~50 ms from a first untimed one.  The
figure is the median of the five windows per call, "spread" the range of the five windows over their median.  Before timing, the
CRCs of the two outputs are compared.  "bound us" is the time the layer's bytes (input + output once) need at 8 TB/s.  Prints a
markdown table; "wins" says whether the new kernel's median lies below the direct kernel's by more than the two spreads TOGETHER
(dw_nchw_kxk.h:dn_default's criterion).

Shapes: the 5x5 depthwise layers of MobileNetV3-Large and EfficientNet-B0 and the 7x7 ones of ConvNeXt-T, both dtypes, batch 1 and 32.
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
HBM_BYTES_PER_US = 8.0e6
NETS = [
    # name, channels, input map, k, stride
    ("mbv3_72_56_s2", 72, 56, 5, 2), ("mbv3_120_28", 120, 28, 5, 1), ("mbv3_672_14", 672, 14, 5, 1), ("mbv3_672_14_s2", 672, 14, 5, 2),
    ("mbv3_960_7", 960, 7, 5, 1),
    ("effb0_144_56_s2", 144, 56, 5, 2), ("effb0_240_28", 240, 28, 5, 1), ("effb0_480_14", 480, 14, 5, 1), ("effb0_1152_7", 1152, 7, 5, 1),
    ("cnxt_96_56", 96, 56, 7, 1), ("cnxt_192_28", 192, 28, 7, 1), ("cnxt_384_14", 384, 14, 7, 1), ("cnxt_768_7", 768, 7, 7, 1),
]
SHAPES = [("%s_b%d_%s" % (name, n, dt), n, dt, c, hw, k, s) for (name, c, hw, k, s) in NETS for n in (1, 32) for dt in ("int8", "f16")]


def worker(a, shapes):
    """one side: per shape `ready <kernel> <crc> <bytes>`, then a window of N replays per `w N` line (its milliseconds back), `n`: next"""
    import cases
    import residual_cases as rc
    pkg = cases.pkg
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("dw_nchw_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()
    for name, n, dt, c, hw, k, s in shapes:
        cv = cases.make_case(9791, layout="NCHW", dtype=dt, depthwise=True, n=n, h=hw, w=hw, c=c, k=(k, k), stride=(s, s), pad=(k // 2,) * 4,
                             exact=False, act=1)
        out_dt = np.int8 if dt == "int8" else np.float16
        count = int(np.prod(cv["out_shape"]))
        plan = rc.make_plan(hip, cv)
        bufs = []
        for _ in range(SETS):
            b = dict(x=dev.alloc(cv["input"].nbytes), y=dev.alloc(count * cv["input"].itemsize))
            dev.upload(b["x"], cv["input"])
            bufs.append(b)

        def enqueue(kk):
            b = bufs[kk % SETS]
            pkg.check(hip.shl_mi355x_conv_forward(plan, b["x"], b["y"], 0, stream), hip, "conv_forward")
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        crc = zlib.crc32(dev.download(bufs[0]["y"], (count,), out_dt).tobytes())
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for kk in range(a.reps):
            enqueue(kk)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("dw_nchw_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
        hip.shl_mi355x_graph_launch(g, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "first replay")
        print("ready", hip.shl_mi355x_conv_plan_kernel_name(plan).decode(), crc, cv["input"].nbytes + count * cv["input"].itemsize, flush=True)
        while True:
            line = sys.stdin.readline()
            if not line:
                raise SystemExit("dw_nchw_bench: the parent went away")  # (the other side failed: nothing more is launched)
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
    sides = [subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=dict(os.environ, SHL_MI355X_DWNCHW=v))
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
            raise SystemExit("dw_nchw_bench: a worker ended early (exit %s)" % p.wait())
        return line.split()

    def figure(windows, calls):
        windows = sorted(windows)
        return windows[2] * 1e-3 / calls, (windows[-1] - windows[0]) / windows[2]

    head = ["shape", "planes x Ho x Wo x taps", "bound us", "direct us", "spread", "kernel at =1", "new us", "spread", "new / direct", "wins"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for name, n, dt, c, hw, k, s in shapes:
        ho = (hw + 2 * (k // 2) - k) // s + 1
        dims = "%d x %d x %d x %d" % (n * c, ho, ho, k * k)
        ready = [ask(p) for p in sides]
        if "direct" not in ready[0][1] or "dwconv_kxk_nchw" not in ready[1][1] or ready[0][2] != ready[1][2]:
            for q in sides:
                q.kill()
            raise SystemExit("dw_nchw_bench: %s: kernels %s / %s, checksums %s / %s" % (name, ready[0][1], ready[1][1], ready[0][2], ready[1][2]))
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
        cells = [name, dims, "%.2f" % (int(ready[0][3]) / HBM_BYTES_PER_US), "%.2f" % (t0 * 1e6), "%.0f %%" % (100 * sp0), ready[1][1],
                 "%.2f" % (t1 * 1e6), "%.0f %%" % (100 * sp1), "%.2f" % (t1 / t0), "yes" if wins else "no"]
        row = "| " + " | ".join(cells) + " |"
        lines.append(row)
        print(row, flush=True)
    for p in sides:
        p.stdin.close()
        if p.wait() != 0:
            raise SystemExit("dw_nchw_bench: a worker failed (exit %d)" % p.returncode)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
