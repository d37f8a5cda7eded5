#!/usr/bin/env python3
"""Windowed pooling kernels against the plain streaming kernel, through the C-ABI (no torch).

    python tools/pool_bench.py [--batch 128] [--reps 12] [--out FILE.md]
Times ResNet-50's pool (N x 112 x 112 x 64, 3x3 stride 2 pad 1) and two MobileNet-size 2x2 stride-2 average pools in
int8 and binary16, NHWC and NCHW: `reps` launches captured in one hipGraph (rotating over three buffer sets, so that a
launch does not find its input in the last-level cache), the graph replayed 20 times between two HIP events, median
of five such windows.  The yardstick, timed the same way in the same process, is shl_mi355x_add on tensors with the
same total bytes (two inputs + output = the pool's input + output).  Prints a markdown table: pool time, add time,
their ratio, algorithmic TB/s (input + output bytes over time).  Before timing, every configuration's output is
compared with the literal one-output-per-thread form (SHL_MI355X_POOL_FORM=generic) on the device's own data.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cases
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("pool_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()

    def timed(enqueue):
        """enqueue(k): the k-th launch on `stream`; seconds per launch"""
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for k in range(a.reps):
            enqueue(k)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("pool_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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
        return sorted(windows)[2] * 1e-3 / (20 * a.reps)

    n = a.batch
    shapes = [("resnet50 pool 112x112x64 k3 s2 p1", "max", 112, 64, 3, 2, 1),
              ("same window, average", "avg", 112, 64, 3, 2, 1),
              ("avg 56x56x128 k2 s2", "avg", 56, 128, 2, 2, 0),
              ("avg 14x14x512 k2 s2", "avg", 14, 512, 2, 2, 0)]
    lines = ["| shape (batch %d) | dtype | layout | kernel | pool us | add us | pool / add | pool TB/s | add TB/s |" % n,
             "|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    for title, kind, hw, c, k, s, p in shapes:
        ho = (hw + 2 * p - k) // s + 1
        for dtype in ("int8", "f16"):
            es = 1 if dtype == "int8" else 2
            in_elems, out_elems = n * hw * hw * c, n * ho * ho * c
            total = (in_elems + out_elems) * es
            # one random block, repeated: the values do not matter for the time, the upload does for the set-up
            block = rng.integers(-128, 128, 1 << 20, dtype=np.int8) if es == 1 else \
                rng.standard_normal(1 << 20).astype(np.float16)
            host = np.tile(block, in_elems // block.size + 1)[:in_elems]
            ins = [dev.alloc(in_elems * es) for _ in range(SETS)]
            outs = [dev.alloc(out_elems * es) for _ in range(SETS)]
            for b in ins:
                dev.upload(b, host)
            # the yardstick: add over count elements, 3 * count * es == total bytes
            count = total // (3 * es)
            abuf = [dev.alloc(count * es) for _ in range(SETS)]

            def add_launch(kk):
                i = kk % SETS
                # input 0: the head of a pool input (count <= in_elems); input 1 and the output: buffers of their own
                pkg.check(hip.shl_mi355x_add(ins[i], abuf[i], abuf[(i + 1) % SETS], count, 0 if es == 1 else 1, 0.05, 3,
                                             0.04, -2, 0.07, 5, stream), hip, "add")
            assert count <= in_elems
            t_add = timed(add_launch)
            for layout in ("NHWC", "NCHW"):
                d = pkg.PoolDesc()
                d.kind = pkg.POOL_MAX if kind == "max" else pkg.POOL_AVG
                d.dtype = pkg.SHL_I8 if es == 1 else pkg.SHL_F16
                d.layout = pkg.SHL_NHWC if layout == "NHWC" else pkg.SHL_NCHW
                d.batch, d.c, d.in_h, d.in_w, d.out_h, d.out_w = n, c, hw, hw, ho, ho
                d.kernel_h = d.kernel_w = k
                d.stride_h = d.stride_w = s
                d.pad_top = d.pad_left = p
                d.in_scale, d.in_zp, d.out_scale, d.out_zp = 0.0473, -9, 0.0219, 4
                name = hip.shl_mi355x_pool2d_kernel_name(C.byref(d)).decode()
                # same answer as the literal form on this data
                pkg.check(hip.shl_mi355x_pool2d(ins[0], outs[0], C.byref(d), stream), hip, "pool2d")
                os.environ["SHL_MI355X_POOL_FORM"] = "generic"
                pkg.check(hip.shl_mi355x_pool2d(ins[0], outs[1], C.byref(d), stream), hip, "pool2d generic")
                del os.environ["SHL_MI355X_POOL_FORM"]
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                got = dev.download(outs[0], (out_elems * es,), np.uint8)
                lit = dev.download(outs[1], (out_elems * es,), np.uint8)
                if not np.array_equal(got, lit):
                    raise SystemExit("pool_bench: %s %s %s: %s differs from the literal form" % (title, dtype, layout, name))

                def pool_launch(kk):
                    pkg.check(hip.shl_mi355x_pool2d(ins[kk % SETS], outs[kk % SETS], C.byref(d), stream), hip, "pool2d")
                t_pool = timed(pool_launch)
                lines.append("| %s | %s | %s | %s | %.1f | %.1f | %.2f | %.2f | %.2f |" % (
                    title, dtype, layout, name, t_pool * 1e6, t_add * 1e6, t_pool / t_add, total / t_pool / 1e12,
                    3 * count * es / t_add / 1e12))
                print(lines[-1], flush=True)
            for b in ins + outs + abuf:
                dev.free(b)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
