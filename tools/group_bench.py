#!/usr/bin/env python3
"""Grouped int8 NCHW convolution on the matrix cores (csrc/conv_group_mfma.hip) against the direct kernel it replaces, through the
C-ABI (no torch); with --dtype f16 the binary16 twin (csrc/conv_group_mfma_f16.hip, switch SHL_MI355X_GROUPMFMA_F16, whose results
differ from the direct kernel's by summation order: the two sides' sum |y| must agree to 1e-3 instead of their CRCs).

    python tools/group_bench.py [--dtype int8|f16] [--reps 4] [--only NAME[,NAME]] [--out FILE.md]
SHL_MI355X_GROUPMFMA is read once per process, so the two sides are two worker processes of this script on the same build: one
under =1 (conv_group_mfma_i8_mfma32x32x32 wherever the geometry fits), one under =0 (exactly the parent commit's code path, the
baseline).  Per shape each worker captures one hipGraph holding `reps` shl_mi355x_conv_forward calls that rotate over three
buffer sets (so that a call does not find its operands in the last-level cache); on the new side a call is three launches -- the
NCHW -> NHWC re-layout, the kernel, the re-layout back -- and all three are in its time.  The parent times the graphs
ALTERNATELY: five rounds, in each a window of replays of the direct graph, then one of the new kernel's, between two HIP events;
a window is sized to ~50 ms from a first untimed one.  The figure is the median of the five windows per call, "spread" the range
of the five windows over their median.  Before timing, the CRCs of the two outputs are compared.  Prints a markdown table;
"wins" says whether the new kernel was faster by more than the larger of the two spreads, the criterion of csrc/lut_validate.h.

Shapes: the grouped 3x3 layers of ResNeXt-50 32x4d at stride 1 and 2 and two RegNetX layers (group width 16: 800MF; 48: 3.2GF,
which is outside the kernel's scope and shows what stays behind), at batch 1 and 32.
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
ALGO_GROUP = 7  # SHL_MI355X_ALGO_GROUP
NETS = [
    # name, input map, C, groups, stride
    ("resnext50_128_56", 56, 128, 32, 1), ("resnext50_128_56_s2", 56, 128, 32, 2),
    ("resnext50_256_28", 28, 256, 32, 1), ("resnext50_256_28_s2", 28, 256, 32, 2),
    ("resnext50_512_14", 14, 512, 32, 1), ("resnext50_512_14_s2", 14, 512, 32, 2),
    ("resnext50_1024_7", 7, 1024, 32, 1), ("resnext50_1024_7_s2", 7, 1024, 32, 2),
    ("resnext101_32x8d_2048_7", 7, 2048, 32, 1), ("resnext101_32x8d_2048_14_s2", 14, 2048, 32, 2),
    ("regnetx800mf_128_28_gw16", 28, 128, 8, 1),
    ("regnetx3.2gf_192_28_gw48", 28, 192, 4, 1),
]
SHAPES = [(name + "_b%d" % n, n, hw, c, g, s) for (name, hw, c, g, s) in NETS for n in (1, 32)]


def worker(a, shapes):
    """one side: per shape `ready <kernel> <crc>`, then a window of N replays per `w N` line (its milliseconds back), `n`: next"""
    import cases
    import residual_cases as rc
    pkg = cases.pkg
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("group_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()
    for name, n, hw, c, groups, stride in shapes:
        cv = cases.make_case(9779, layout="NCHW", dtype=a.dtype, n=n, h=hw, w=hw, c=c, co=c, groups=groups, stride=(stride, stride), exact=False, act=1)
        count = int(np.prod(cv["out_shape"]))
        desc, plan = rc.conv_desc(cv), C.c_void_p()
        desc.algo = ALGO_GROUP
        mult = (np.float32(cv["in_scale"]) * np.broadcast_to(cv["k_scale"], (c,))).astype(np.float32)
        bias = (cv["bias"].astype(np.float32) * np.broadcast_to(cv["b_scale"], (c,))).astype(np.float32)
        pkg.check(hip.shl_mi355x_conv_plan_create(C.byref(desc), cv["kernel"].ctypes.data, mult.ctypes.data, bias.ctypes.data, None,
                                                  C.byref(plan)), hip, "conv_plan_create")
        bufs = []
        for _ in range(SETS):
            b = dict(x=dev.alloc(cv["input"].nbytes), y=dev.alloc(count * (2 if a.dtype == "f16" else 1)))
            dev.upload(b["x"], cv["input"])
            bufs.append(b)

        def enqueue(kk):
            b = bufs[kk % SETS]
            pkg.check(hip.shl_mi355x_conv_forward(plan, b["x"], b["y"], 0, stream), hip, "conv_forward")
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        if a.dtype == "f16":  # (summation order differs between the two kernels: a norm instead of a CRC)
            crc = "%.6e" % float(np.abs(dev.download(bufs[0]["y"], (count,), np.float16).astype(np.float64)).sum())
        else:
            crc = zlib.crc32(dev.download(bufs[0]["y"], (count,), np.int8).tobytes())
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for kk in range(a.reps):
            enqueue(kk)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("group_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
        hip.shl_mi355x_graph_launch(g, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "first replay")
        print("ready", hip.shl_mi355x_conv_plan_kernel_name(plan).decode(), crc, flush=True)
        while True:
            line = sys.stdin.readline()
            if not line:
                raise SystemExit("group_bench: the parent went away")  # (the other side failed: nothing more is launched)
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
    ap.add_argument("--dtype", default="int8", choices=("int8", "f16"))
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    shapes = [s for s in SHAPES if not only or s[0] in only]
    if a.worker:
        return worker(a, shapes)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps), "--only", a.only, "--dtype", a.dtype]
    switch = "SHL_MI355X_GROUPMFMA" if a.dtype == "int8" else "SHL_MI355X_GROUPMFMA_F16"
    sides = [subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=dict(os.environ, **{switch: v}))
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
            raise SystemExit("group_bench: a worker ended early (exit %s)" % p.wait())
        return line.split()

    def figure(windows, calls):
        windows = sorted(windows)
        return windows[2] * 1e-3 / calls, (windows[-1] - windows[0]) / windows[2]

    head = ["shape", "M x C / G x taps", "direct us", "spread", "kernel at =1", "new us (3 launches)", "spread", "new / direct", "wins"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for name, n, hw, c, groups, stride in shapes:
        ho = (hw + 2 - 3) // stride + 1
        dims = "%d x %d / %d x 9" % (n * ho * ho, c, groups)
        ready = [ask(p) for p in sides]
        same = ready[0][2] == ready[1][2] if a.dtype == "int8" else abs(float(ready[0][2]) - float(ready[1][2])) <= 1e-3 * float(ready[0][2])
        if ready[0][1] != "conv_group_direct_" + ("i8" if a.dtype == "int8" else "f16") or not same:
            raise SystemExit("group_bench: %s: baseline kernel %s, checksums %s / %s" % (name, ready[0][1], ready[0][2], ready[1][2]))
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
            raise SystemExit("group_bench: a worker failed (exit %d)" % p.returncode)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
