#!/usr/bin/env python3
"""The table kernel, the binary16 unary kernel and the mul forms against the existing relu / add kernels, through the C-ABI
(no torch).

    python tools/eltwise_bench.py [--reps 12] [--out FILE.md] [--sizes small,large]
Sizes: 1 x 112 x 112 x 32 (the batch-1 size) and 128 x 56 x 56 x 64 (the bandwidth size).  Every row is `reps` launches
captured in one hipGraph (rotating over three buffer sets, so that a launch does not find its input in the last-level
cache), the graph replayed 20 times between two HIP events, median of five such windows: 240 launches per window at the
default.  Yardsticks, timed the same way in the same process on equal bytes: shl_mi355x_relu_i8 / _relu_f16 for the unary
kernels, shl_mi355x_add for mul.  Prints a markdown table: time, the yardstick's time, their ratio, algorithmic TB/s
(bytes read + written over time).  Before timing, every mul form's output is compared with the literal
one-output-per-thread form (SHL_MI355X_MUL_FORM=generic), and the table kernel's with relu_i8's through a relu table.
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
SIZES = {"small": (1, 112, 112, 32), "large": (128, 56, 56, 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="small,large")
    a = ap.parse_args()
    import cases
    import eltwise_cases
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("eltwise_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
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
            raise SystemExit("eltwise_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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

    lines = ["| size | dtype | kernel | operands | us | yardstick | yardstick us | ratio | TB/s | yardstick TB/s |",
             "|---|---|---|---|---|---|---|---|---|---|"]

    def row(size, dtype, kernel, operands, t, nbytes, yard, t_yard, yard_bytes):
        lines.append("| %s | %s | %s | %s | %.1f | %s | %.1f | %.2f | %.2f | %.2f |" % (
            "x".join(map(str, size)), dtype, kernel, operands, t * 1e6, yard, t_yard * 1e6, t / t_yard, nbytes / t / 1e12,
            yard_bytes / t_yard / 1e12))
        print(lines[-1], flush=True)

    rng = np.random.default_rng(1)
    in_q, out_q = (0.0473, -9), (0.0219, 4)
    for key in a.sizes.split(","):
        size = SIZES[key]
        n, h, w, c = size
        count = n * h * w * c
        for dtype in ("int8", "f16"):
            es = 1 if dtype == "int8" else 2
            code = pkg.SHL_I8 if es == 1 else pkg.SHL_F16
            # one random block, repeated: the values do not matter for the time, the upload does for the set-up
            block = rng.integers(-128, 128, 1 << 20, dtype=np.int8) if es == 1 else rng.standard_normal(1 << 20).astype(np.float16)
            pad = 64  # room for the pointer one element off the grid
            xs = [dev.alloc(count * es + pad) for _ in range(SETS)]
            ys = [dev.alloc(count * es + pad) for _ in range(SETS)]
            outs = [dev.alloc(count * es + pad) for _ in range(SETS)]
            for b in xs + ys:
                dev.upload(b, np.tile(block, count // block.size + 1)[:count])

            def download(p):
                return dev.download(p, (count * es,), np.uint8)
            # ---- unary
            if es == 1:
                def relu(kk):
                    i = kk % SETS
                    pkg.check(hip.shl_mi355x_relu_i8(xs[i], outs[i], count, in_q[0], in_q[1], out_q[0], out_q[1], 0, stream), hip, "relu_i8")
                t_relu = timed(relu)
                # a relu table (the reference's formula on the host, in numpy): the table kernel must give relu_i8's bytes
                q = np.arange(-128, 128, dtype=np.int16).astype(np.int8)
                f = eltwise_cases.pool_cases.dequantise(q, "int8", in_q)
                tab = eltwise_cases.pool_cases.requantise(np.maximum(f, np.float32(0)), "int8", out_q)
                table = np.zeros(256, np.uint8)
                table[q.view(np.uint8)] = tab.view(np.uint8)
                tptr = table.ctypes.data
                for off, label in ((0, "aligned"), (1, "input + 1 byte")):
                    def lut(kk, off=off):
                        i = kk % SETS
                        pkg.check(hip.shl_mi355x_unary_lut_i8(xs[i] + off, outs[i], count, tptr, stream), hip, "unary_lut_i8")
                    if off == 0:
                        relu(0)
                        lut(1)
                        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                        if not np.array_equal(download(outs[0]), download(outs[1])):
                            raise SystemExit("eltwise_bench: the table kernel differs from relu_i8")
                    name = hip.shl_mi355x_unary_lut_i8_kernel_name(xs[0] + off, outs[0]).decode()
                    row(size, dtype, name, label, timed(lut), 2 * count, "relu_i8", t_relu, 2 * count)
            else:
                def relu(kk):
                    i = kk % SETS
                    pkg.check(hip.shl_mi355x_relu_f16(xs[i], outs[i], count, 0, stream), hip, "relu_f16")
                t_relu = timed(relu)
                for op, kind in eltwise_cases.KIND.items():
                    def unary(kk, kind=kind):
                        i = kk % SETS
                        pkg.check(hip.shl_mi355x_unary_f16(xs[i], outs[i], count, kind, 0.1, stream), hip, "unary_f16")
                    row(size, dtype, "unary_f16", op, timed(unary), 4 * count, "relu_f16", t_relu, 4 * count)
            # ---- mul
            def add(kk):
                i = kk % SETS
                pkg.check(hip.shl_mi355x_add(xs[i], ys[i], outs[i], count, code, 0.05, 3, 0.04, -2, 0.07, 5, stream), hip, "add")
            t_add = timed(add)
            case = dict(dtype=dtype, in_q=(0.05, 3), in1_q=(0.04, -2), out_q=(0.07, 5))
            shapes = [("same shape", (n, h, w, c), (n, h, w, c)), ("NHWC x [N,1,1,C]", (n, h, w, c), (n, 1, 1, c)),
                      ("x [C]", (n, h, w, c), (c,)), ("x scalar", (n, h, w, c), (1,)),
                      ("NCHW x [N,C,1,1]", (n, c, h, w), (n, c, 1, 1)), ("NCHW x [1,C,1,1]", (n, c, h, w), (1, c, 1, 1))]
            for label, a_shape, b_shape in shapes:
                d = eltwise_cases.mul_desc(case, a_shape, b_shape)
                b_bytes = int(np.prod(b_shape)) * es

                def mul(kk, d=d, what="mul"):
                    i = kk % SETS
                    pkg.check(hip.shl_mi355x_mul(xs[i], ys[i], outs[i], C.byref(d), stream), hip, what)
                mul(0)
                os.environ["SHL_MI355X_MUL_FORM"] = "generic"
                mul(1, what="mul generic")
                del os.environ["SHL_MI355X_MUL_FORM"]
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                if not np.array_equal(download(outs[0]), download(outs[1])):
                    raise SystemExit("eltwise_bench: mul %s %s differs from the literal form" % (dtype, label))
                for force in (("", "generic") if label in ("NHWC x [N,1,1,C]", "NCHW x [N,C,1,1]") else ("",)):
                    if force:
                        os.environ["SHL_MI355X_MUL_FORM"] = force
                    name = hip.shl_mi355x_mul_kernel_name(C.byref(d), xs[0], ys[0], outs[0]).decode()
                    t = timed(mul)
                    os.environ.pop("SHL_MI355X_MUL_FORM", None)
                    row(size, dtype, name, label, t, 2 * count * es + b_bytes, "add", t_add, 3 * count * es)
            for b in xs + ys + outs:
                dev.free(b)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
