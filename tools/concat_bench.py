#!/usr/bin/env python3
"""The concat kernels against the plain streaming kernel, through the C-ABI (no torch).

    python tools/concat_bench.py [--batch 128] [--reps 12] [--out FILE.md]
Times SqueezeNet's fire2 concat (N x 55 x 55 x (64 + 64)) and GoogLeNet's inception-3a concat of four branches
(N x 28 x 28 x (64 + 128 + 32 + 32)) in int8 and binary16, NHWC (outer = N H W, rows of C_i) and NCHW (outer = N, rows of
C_i H W), in each kernel form: `reps` launches captured in one hipGraph (rotating over three buffer sets, so that a launch
does not find its input in the last-level cache), the graph replayed 20 times between two HIP events, median of five such
windows.  int8 runs the vector form twice: with every input record equal to the output's (raw copies) and with records
of their own (sixteen requantisations per thread).  The yardstick, timed the same way in the same process, is
shl_mi355x_add on tensors with the same total bytes (two inputs + output = the concat's inputs + output).  Prints a
markdown table: concat time, add time, their ratio, algorithmic TB/s (input + output bytes over time).  Before timing,
every configuration's output is compared with the literal one-element-per-thread form (SHL_MI355X_CONCAT_FORM=generic)
on the device's own data.
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
        raise SystemExit("concat_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
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
            raise SystemExit("concat_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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
    shapes = [("fire2 55x55x(64+64)", 55, (64, 64)), ("inception-3a 28x28x(64+128+32+32)", 28, (64, 128, 32, 32))]
    out_q = (0.0625, -5)
    own = [(0.0473, -9), (0.0311, 3), (0.0127, -20), (0.0219, 4)]
    lines = ["| shape (batch %d) | dtype | layout | kernel | records | concat us | add us | concat / add | concat TB/s | add TB/s |" % n,
             "|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    for title, hw, cs in shapes:
        for dtype in ("int8", "f16"):
            es = 1 if dtype == "int8" else 2
            elems = [n * hw * hw * c for c in cs]
            out_elems = sum(elems)
            total = 2 * out_elems * es
            # one random block, repeated: the values do not matter for the time, the upload does for the set-up
            block = rng.integers(-128, 128, 1 << 20, dtype=np.int8) if es == 1 else \
                rng.standard_normal(1 << 20).astype(np.float16)
            ins = [[dev.alloc(e * es) for e in elems] for _ in range(SETS)]
            outs = [dev.alloc(out_elems * es) for _ in range(SETS)]
            for bufs in ins:
                for b, e in zip(bufs, elems):
                    dev.upload(b, np.tile(block, e // block.size + 1)[:e])
            # the yardstick: add over count elements, 3 * count * es == total bytes (its operands: the heads of the outputs)
            count = total // (3 * es)
            assert count <= out_elems

            def add_launch(kk):
                i = kk % SETS
                pkg.check(hip.shl_mi355x_add(outs[i], outs[(i + 1) % SETS], outs[(i + 2) % SETS], count, 0 if es == 1 else 1,
                                             0.05, 3, 0.04, -2, 0.07, 5, stream), hip, "add")
            t_add = timed(add_launch)
            for layout in ("NHWC", "NCHW"):
                outer = n * hw * hw if layout == "NHWC" else n
                lens = [e // outer for e in elems]
                for records in (("equal", "own") if es == 1 else ("-",)):
                    qs = own[:len(cs)] if records == "own" else [out_q] * len(cs)
                    d = pkg.ConcatDesc()
                    d.dtype = pkg.SHL_I8 if es == 1 else pkg.SHL_F16
                    d.n_inputs, d.outer = len(cs), outer
                    d.out_scale, d.out_zp = out_q
                    c_len = (C.c_int64 * len(cs))(*lens)
                    c_s = (C.c_float * len(cs))(*[q[0] for q in qs])
                    c_z = (C.c_int32 * len(cs))(*[q[1] for q in qs])
                    c_in = [(C.c_void_p * len(cs))(*bufs) for bufs in ins]

                    def launch(kk, what="concat"):
                        i = kk % SETS
                        pkg.check(hip.shl_mi355x_concat(c_in[i], c_len, c_s, c_z, outs[i], C.byref(d), stream), hip, what)
                    # same answer as the literal form on this data
                    launch(0)
                    os.environ["SHL_MI355X_CONCAT_FORM"] = "generic"
                    launch(1, "concat generic")
                    del os.environ["SHL_MI355X_CONCAT_FORM"]
                    pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                    got = dev.download(outs[0], (out_elems * es,), np.uint8)
                    lit = dev.download(outs[1], (out_elems * es,), np.uint8)
                    if not np.array_equal(got, lit):
                        raise SystemExit("concat_bench: %s %s %s %s differs from the literal form" % (title, dtype, layout, records))
                    # the literal form requantises whatever the records are: timed once per dtype and layout
                    for force in ([""] if records == "equal" else ["", "generic"]):
                        if force:
                            os.environ["SHL_MI355X_CONCAT_FORM"] = force
                        name = hip.shl_mi355x_concat_kernel_name(c_in[0], c_len, c_s, c_z, outs[0], C.byref(d)).decode()
                        t = timed(launch)
                        os.environ.pop("SHL_MI355X_CONCAT_FORM", None)
                        lines.append("| %s | %s | %s | %s | %s | %.1f | %.1f | %.2f | %.2f | %.2f |" % (
                            title, dtype, layout, name, records, t * 1e6, t_add * 1e6, t / t_add, total / t / 1e12,
                            3 * count * es / t_add / 1e12))
                        print(lines[-1], flush=True)
            for b in [p for bufs in ins for p in bufs] + outs:
                dev.free(b)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
