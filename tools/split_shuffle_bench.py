#!/usr/bin/env python3
"""The split and shuffle_channel kernels against the plain streaming kernel, through the C-ABI (no torch).

    python tools/split_shuffle_bench.py [--batches 1,128] [--reps 12] [--out FILE.md]
Times ShuffleNetV2 1x's own shapes -- a unit's split into two halves of 58 / 116 / 232 channels and its shuffle_channel
(two groups) of 116 / 232 / 464 channels at 28 / 14 / 7 -- at batch 1 and 128, in int8 and binary16, NHWC (outer = N H W) and
NCHW (outer = N), in every kernel form the shape admits: `reps` launches captured in one hipGraph (rotating over three
buffer sets, so that a launch does not find its input in the last-level cache), the graph replayed 20 times between two
HIP events, median of five such windows.  int8 runs twice: with the output records equal to the input's (raw copies) and
with records of their own (a requantisation per element).  The yardstick, timed the same way in the same process, is the
streaming shl_mi355x_relu_i8 / _f16 on the same number of elements: it reads and writes exactly the bytes the operator
moves.  Prints a markdown table: time, relu time, their ratio, algorithmic GB/s (input + output bytes over time).  Before
timing, every configuration's output is compared with the literal one-element-per-thread form on the device's own data.
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
ENV = {"split": "SHL_MI355X_SPLIT_FORM", "shuffle": "SHL_MI355X_SHUFFLE_FORM"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,128")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cases
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("split_shuffle_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
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
            raise SystemExit("split_shuffle_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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

    in_q, own = (0.0625, -5), [(0.0473, -9), (0.0311, 3)]
    lines = ["| op | shape | batch | dtype | layout | kernel | records | us | relu us | op / relu | GB/s | relu GB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    for n in [int(v) for v in a.batches.split(",")]:
        for half, hw in ((58, 28), (116, 14), (232, 7)):
            c = 2 * half
            for dtype in ("int8", "f16"):
                es = 1 if dtype == "int8" else 2
                elems = n * hw * hw * c
                total = 2 * elems * es
                block = rng.integers(-128, 128, 1 << 20, dtype=np.int8) if es == 1 else rng.standard_normal(1 << 20).astype(np.float16)
                ins = [dev.alloc(elems * es) for _ in range(SETS)]
                outs = [[dev.alloc(elems * es // 2) for _ in range(2)] for _ in range(SETS)]   # a split's halves
                whole = [dev.alloc(elems * es) for _ in range(SETS)]                           # a shuffle's output
                for b in ins:
                    dev.upload(b, np.tile(block, elems // block.size + 1)[:elems])

                def relu_launch(kk):
                    i = kk % SETS
                    if es == 1:
                        pkg.check(hip.shl_mi355x_relu_i8(ins[i], whole[i], elems, 0.05, 3, 0.04, -2, 0, stream), hip, "relu")
                    else:
                        pkg.check(hip.shl_mi355x_relu_f16(ins[i], whole[i], elems, 0, stream), hip, "relu")
                t_relu = timed(relu_launch)
                for layout in ("NHWC", "NCHW"):
                    outer, inner = (n * hw * hw, 1) if layout == "NHWC" else (n, hw * hw)
                    for records in (("equal", "own") if es == 1 else ("-",)):
                        qs = own if records == "own" else [in_q] * 2
                        sd = pkg.SplitDesc()
                        sd.dtype = pkg.SHL_I8 if es == 1 else pkg.SHL_F16
                        sd.n_outputs, sd.outer = 2, outer
                        sd.in_scale, sd.in_zp = in_q
                        s_len = (C.c_int64 * 2)(half * inner, half * inner)
                        s_s = (C.c_float * 2)(*[q[0] for q in qs])
                        s_z = (C.c_int32 * 2)(*[q[1] for q in qs])
                        s_out = [(C.c_void_p * 2)(*bufs) for bufs in outs]
                        hd = pkg.ShuffleDesc()
                        hd.dtype, hd.group, hd.outer, hd.c, hd.inner = sd.dtype, 2, outer, c, inner
                        hd.in_scale, hd.in_zp = in_q
                        hd.out_scale, hd.out_zp = qs[0]

                        def split_launch(kk, what="split"):
                            i = kk % SETS
                            pkg.check(hip.shl_mi355x_split(ins[i], s_out[i], s_len, s_s, s_z, C.byref(sd), stream), hip, what)

                        def shuffle_launch(kk, what="shuffle_channel"):
                            i = kk % SETS
                            pkg.check(hip.shl_mi355x_shuffle_channel(ins[i], whole[i], C.byref(hd), stream), hip, what)

                        def fetch(op, i):
                            if op == "split":
                                return np.concatenate([dev.download(p, (elems * es // 2,), np.uint8) for p in outs[i]])
                            return dev.download(whole[i], (elems * es,), np.uint8)
                        for op, launch, forces in (("split", split_launch, ["", "generic"]),
                                                   ("shuffle", shuffle_launch, ["", "generic"])):
                            # same answer as the literal form on this data (every set holds the same input)
                            launch(0)
                            os.environ[ENV[op]] = "generic"
                            launch(1, op + " generic")
                            del os.environ[ENV[op]]
                            pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                            if not np.array_equal(fetch(op, 0), fetch(op, 1)):
                                raise SystemExit("split_shuffle_bench: %s %dx%dx%d batch %d %s %s %s differs from the literal form"
                                                 % (op, hw, hw, c, n, dtype, layout, records))
                            seen = set()
                            for force in forces:
                                if force:
                                    os.environ[ENV[op]] = force
                                if op == "split":
                                    name = hip.shl_mi355x_split_kernel_name(ins[0], s_out[0], s_len, s_s, s_z, C.byref(sd)).decode()
                                else:
                                    name = hip.shl_mi355x_shuffle_channel_kernel_name(ins[0], whole[0], C.byref(hd)).decode()
                                # the literal form requantises whatever the records are: timed once per dtype and layout
                                if name in seen or (name.endswith("generic") and records == "equal" and force):
                                    os.environ.pop(ENV[op], None)
                                    continue
                                seen.add(name)
                                t = timed(launch)
                                os.environ.pop(ENV[op], None)
                                shape = "%dx%dx(%d+%d)" % (hw, hw, half, half) if op == "split" else "%dx%dx%d g2" % (hw, hw, c)
                                lines.append("| %s | %s | %d | %s | %s | %s | %s | %.2f | %.2f | %.2f | %.0f | %.0f |" % (
                                    op, shape, n, dtype, layout, name, records, t * 1e6, t_relu * 1e6, t / t_relu,
                                    total / t / 1e9, total / t_relu / 1e9))
                                print(lines[-1], flush=True)
                for b in ins + whole + [p for bufs in outs for p in bufs]:
                    dev.free(b)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
