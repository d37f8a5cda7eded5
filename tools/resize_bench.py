#!/usr/bin/env python3
"""Resize kernels against the plain streaming kernel, through the C-ABI (no torch).

    python tools/resize_bench.py [--batch 128] [--reps 12] [--out FILE.md]
Times a 2x upsample of N x 14 x 14 x 512, N x 28 x 28 x 256 and N x 56 x 56 x 128 in int8 and binary16, NHWC and NCHW,
nearest and bilinear: `reps` launches captured in one hipGraph (rotating over three buffer sets, so that a launch does
not find its input in the last-level cache), the graph replayed 20 times between two HIP events, median of five such
windows (the pools' method, profiles/pool2d_notes.md).  The yardstick, timed the same way in the same process, is the
streaming relu of the same dtype on tensors with the same total bytes (input + output = the resize's input + output).
Every configuration is first compared, and then timed, against the literal one-output-per-thread form
(SHL_MI355X_RESIZE_FORM=generic) on the device's own data.  Prints a markdown table: resize time, the literal form's,
relu's, the ratios, algorithmic TB/s (input + output bytes over time), and the spread of the five windows.
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
    import resize_cases
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("resize_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
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
            raise SystemExit("resize_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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

    n = a.batch
    shapes = [(14, 512), (28, 256), (56, 128)]
    lines = ["| 2x of (batch %d) | dtype | layout | mode | kernel | us | literal us | relu us | / relu | literal / kernel | TB/s | spread |" % n,
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    for hw, c in shapes:
        ho = 2 * hw
        for dtype in ("int8", "f16"):
            es = 1 if dtype == "int8" else 2
            in_elems, out_elems = n * hw * hw * c, n * ho * ho * c
            total = (in_elems + out_elems) * es
            # one random block, repeated: the values do not matter for the time, the upload does for the set-up
            block = rng.integers(-128, 128, 1 << 20, dtype=np.int8) if es == 1 else rng.standard_normal(1 << 20).astype(np.float16)
            host = np.tile(block, in_elems // block.size + 1)[:in_elems]
            ins = [dev.alloc(in_elems * es) for _ in range(SETS)]
            outs = [dev.alloc(out_elems * es) for _ in range(SETS)]
            for b in ins:
                dev.upload(b, host)
            # the yardstick: relu over count elements, 2 * count * es == total bytes; it reads the head of one resize output
            # and writes the head of another
            count = total // (2 * es)
            assert count <= out_elems

            def relu_launch(kk):
                i = kk % SETS
                if es == 1:
                    pkg.check(hip.shl_mi355x_relu_i8(outs[i], outs[(i + 1) % SETS], count, 0.0473, -9, 0.0219, 4, 0, stream), hip, "relu")
                else:
                    pkg.check(hip.shl_mi355x_relu_f16(outs[i], outs[(i + 1) % SETS], count, 0, stream), hip, "relu")
            t_relu, _ = timed(relu_launch)
            for layout in ("NHWC", "NCHW"):
                for mode in ("nearest", "bilinear"):
                    case = dict(dtype=dtype, layout=layout, n=n, c=c, h=hw, w=hw, ho=ho, wo=ho, mode=mode, align=False,
                                in_q=(0.0473, -9) if es == 1 else (1.0, 0), out_q=(0.0219, 4) if es == 1 else (1.0, 0))
                    d = resize_cases.resize_desc(case)
                    name = hip.shl_mi355x_resize_kernel_name(C.byref(d), ins[0], outs[0]).decode()

                    def launch(kk):
                        pkg.check(hip.shl_mi355x_resize(ins[kk % SETS], outs[kk % SETS], C.byref(d), stream), hip, "resize")
                    # same answer as the literal form on this data
                    launch(0)
                    os.environ["SHL_MI355X_RESIZE_FORM"] = "generic"
                    pkg.check(hip.shl_mi355x_resize(ins[0], outs[1], C.byref(d), stream), hip, "resize generic")
                    del os.environ["SHL_MI355X_RESIZE_FORM"]
                    pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                    got = dev.download(outs[0], (out_elems * es,), np.uint8)
                    lit = dev.download(outs[1], (out_elems * es,), np.uint8)
                    if not np.array_equal(got, lit):
                        raise SystemExit("resize_bench: %dx%dx%d %s %s %s: %s differs from the literal form" % (hw, hw, c, dtype, layout, mode, name))
                    t, spread = timed(launch)
                    os.environ["SHL_MI355X_RESIZE_FORM"] = "generic"   # read per call: the capture holds the literal kernel
                    t_lit, spread_lit = timed(launch)
                    del os.environ["SHL_MI355X_RESIZE_FORM"]
                    lines.append("| %dx%dx%d | %s | %s | %s | %s | %.1f | %.1f | %.1f | %.2f | %.2f | %.2f | %.0f %% / %.0f %% |" % (
                        hw, hw, c, dtype, layout, mode, name, t * 1e6, t_lit * 1e6, t_relu * 1e6, t / t_relu, t_lit / t,
                        total / t / 1e12, 100 * spread, 100 * spread_lit))
                    print(lines[-1], flush=True)
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
