#!/usr/bin/env python3
"""The reduction kernels against the plain streaming kernel, the global average pool and their own literal form, through the
C-ABI (no torch).

    python tools/reduce_bench.py [--batch 1,128] [--reps 8] [--out FILE.md]
Times, in int8 and binary16, at every batch given:
  * a TensorFlow MobileNetV2 tail's mean over H and W: 7x7x1280 NHWC (cols) and 1280x7x7 NCHW (rows),
  * CBAM's spatial attention on a 56x56x64 map, max and mean over the channel axis in both layouts,
  * global_maxpool2d on the same tail,
  * reduce_max over 1000 classes,
each in the form the rule chooses and forced to the literal form (SHL_MI355X_REDUCE_FORM=generic); and, once, a single row of
2^18 elements: one lane's chain, reported per element.
Each `reps` launches captured in one hipGraph (rotating over three buffer sets, so that a launch does not find its input in
the last-level cache), the graph replayed 20 times between two HIP events, median of five such windows.  Yardsticks, timed the
same way in the same process: the streaming shl_mi355x_relu_i8 / _f16 on the reduction's INPUT bytes (it also writes as many,
which the reduction does not), and for the H, W means shl_mi355x_global_avgpool2d on the same tensor.  Prints a markdown
table.  Before timing, every configuration's output is compared with the literal form's on the device's own data.
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
ENV = "SHL_MI355X_REDUCE_FORM"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="1,128")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cases
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("reduce_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()

    def timed(enqueue, reps):
        """enqueue(k): the k-th launch on `stream`; seconds per launch"""
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for k in range(reps):
            enqueue(k)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("reduce_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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
        return sorted(windows)[2] * 1e-3 / (20 * reps)

    in_q, out_q = (0.0473, -9), (0.0219, 4)
    work = []  # (label, kind, init, shape, reduced axes, global_avgpool2d's (layout, channels, pixels) | None, reps)
    for n in [int(v) for v in a.batch.split(",")]:
        work.append(("mean HW 7x7x1280 NHWC b%d" % n, pkg.REDUCE_MEAN, 0, (n, 7, 7, 1280), (1, 2), (pkg.SHL_NHWC, 1280, 49), a.reps))
        work.append(("mean HW 1280x7x7 NCHW b%d" % n, pkg.REDUCE_MEAN, 0, (n, 1280, 7, 7), (2, 3), (pkg.SHL_NCHW, 1280, 49), a.reps))
        work.append(("gmp 7x7x1280 NHWC b%d" % n, pkg.REDUCE_MAX, 0, (n, 7, 7, 1280), (1, 2), None, a.reps))
        work.append(("gmp 1280x7x7 NCHW b%d" % n, pkg.REDUCE_MAX, 0, (n, 1280, 7, 7), (2, 3), None, a.reps))
        for kind, what in ((pkg.REDUCE_MAX, "max"), (pkg.REDUCE_MEAN, "mean")):
            work.append(("cbam %s C 56x56x64 NHWC b%d" % (what, n), kind, 0, (n, 56, 56, 64), (3,), None, a.reps))
            work.append(("cbam %s C 64x56x56 NCHW b%d" % (what, n), kind, 0, (n, 64, 56, 56), (1,), None, a.reps))
        work.append(("reduce_max 1000 classes b%d" % n, pkg.REDUCE_MAX, 1, (n, 1000), (1,), None, a.reps))
    work.append(("one row of 2^18 (sum)", pkg.REDUCE_SUM, 0, (1, 1 << 18), (1,), None, 1))
    work.append(("one row of 2^18 (max)", pkg.REDUCE_MAX, 0, (1, 1 << 18), (1,), None, 1))
    lines = ["| layer | dtype | kernel | us | relu us | op / relu | input GB/s | ns per inner element | global_avgpool2d us | op / gap |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    for label, kind, init, shape, axes, gap, reps in work:
        for dtype in ("int8", "f16"):
            es = 1 if dtype == "int8" else 2
            in_elems = int(np.prod(shape, dtype=np.int64))
            groups = pkg.reduce_groups(shape, axes)
            out_elems = int(np.prod(groups[0], dtype=np.int64))
            inner = int(np.prod(groups[2], dtype=np.int64))
            block = rng.integers(-128, 128, 1 << 20, dtype=np.int8) if es == 1 else rng.standard_normal(1 << 20).astype(np.float16)
            ins = [dev.alloc(in_elems * es) for _ in range(SETS)]
            outs = [dev.alloc(max(in_elems, out_elems) * es) for _ in range(SETS)]
            for b in ins:
                dev.upload(b, np.tile(block, in_elems // block.size + 1)[:in_elems])
            d = pkg.ReduceDesc()
            d.dtype = pkg.SHL_I8 if es == 1 else pkg.SHL_F16
            d.kind, d.init, d.in_elems = kind, init, in_elems
            d.n_out, d.n_inner = len(groups[0]), len(groups[2])
            for k in range(d.n_out):
                d.out_extent[k], d.out_stride[k] = groups[0][k], groups[1][k]
            for k in range(d.n_inner):
                d.inner_extent[k], d.inner_stride[k] = groups[2][k], groups[3][k]
            (d.in_scale, d.in_zp), (d.out_scale, d.out_zp) = (in_q, out_q) if es == 1 else ((1.0, 0), (1.0, 0))

            def relu_launch(kk):
                i = kk % SETS
                if es == 1:
                    pkg.check(hip.shl_mi355x_relu_i8(ins[i], outs[i], in_elems, 0.05, 3, 0.04, -2, 0, stream), hip, "relu")
                else:
                    pkg.check(hip.shl_mi355x_relu_f16(ins[i], outs[i], in_elems, 0, stream), hip, "relu")
            t_relu = timed(relu_launch, reps)
            t_gap = None
            if gap is not None:
                def gap_launch(kk):
                    i = kk % SETS
                    pkg.check(hip.shl_mi355x_global_avgpool2d(ins[i], outs[i], d.dtype, gap[0], shape[0], gap[1], gap[2], d.in_scale, d.in_zp,
                                                              d.out_scale, d.out_zp, stream), hip, "global_avgpool2d")
                t_gap = timed(gap_launch, reps)

            def launch(kk):
                i = kk % SETS
                pkg.check(hip.shl_mi355x_reduce(ins[i], outs[i], C.byref(d), stream), hip, "reduce")
            os.environ[ENV] = "generic"
            launch(1)
            pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
            literal = dev.download(outs[1], (out_elems * es,), np.uint8)
            del os.environ[ENV]
            for force in ("", "generic"):
                if force:
                    os.environ[ENV] = force
                kernel = hip.shl_mi355x_reduce_kernel_name(ins[0], outs[0], C.byref(d)).decode()
                launch(0)
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                if not np.array_equal(dev.download(outs[0], (out_elems * es,), np.uint8), literal):
                    raise SystemExit("reduce_bench: %s %s %s differs from the literal form" % (label, dtype, kernel))
                t = timed(launch, reps)
                os.environ.pop(ENV, None)
                lines.append("| %s | %s | %s | %.2f | %.2f | %.2f | %.0f | %.3f | %s | %s |" % (
                    label, dtype, kernel, t * 1e6, t_relu * 1e6, t / t_relu, in_elems * es / t / 1e9, t * 1e9 / inner,
                    "%.2f" % (t_gap * 1e6) if t_gap else "-", "%.2f" % (t / t_gap) if t_gap else "-"))
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
