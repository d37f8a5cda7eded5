#!/usr/bin/env python3
"""The transpose, pad and flat-move kernels against the plain streaming kernel and the re-layout pass, through the C-ABI (no
torch).

    python tools/move_bench.py [--batch 128] [--reps 8] [--out FILE.md]
Times, in int8 and binary16, in every kernel form the shape admits (SHL_MI355X_TRANSPOSE_FORM / SHL_MI355X_PAD_FORM):
  * ResNet-50's maps NCHW -> NHWC and back (256 @56, 512 @28, 1024 @14, 2048 @7),
  * a YOLO head [N, 3, 85, 20, 20] -> (0, 1, 3, 4, 2),
  * an attention block's head merge [N, 197, 12, 64] -> (0, 2, 1, 3),
  * TensorFlow's SAME pad (0 before, 1 after on H and W, NHWC) in front of MobileNetV1's stride-2 layers,
  * the classifier tail's flatten [N, 1, 1, 1024], and the same flat move over a 512 @28 map (51 MB in int8),
each `reps` launches captured in one hipGraph (rotating over three buffer sets, so that a launch does not find its input in
the last-level cache), the graph replayed 20 times between two HIP events, median of five such windows.  int8 runs twice:
with the output record equal to the input's (raw copies) and with a record of its own (a requantisation per element).
Yardsticks, timed the same way in the same process: the streaming shl_mi355x_relu_i8 / _f16 on (input + output bytes) / 2 --
it reads and writes exactly the bytes the operator moves -- and, for the batched 2-d transposes, shl_mi355x_layout_convert
(csrc/layout.hip) on the same shape.  Prints a markdown table.  Before timing, every configuration's output is compared with
the literal one-element-per-thread form on the device's own data.
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
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cases
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("move_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
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
            raise SystemExit("move_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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
    in_q, own = (0.0625, -5), (0.0473, -9)
    # (label, op, input shape, permutation | (before, after) | None, layout_convert's (channels, pixels, to_nhwc) | None)
    work = []
    for c, hw in ((256, 56), (512, 28), (1024, 14), (2048, 7)):
        work.append(("resnet50 %d@%d to NHWC" % (c, hw), "transpose", (n, c, hw, hw), (0, 2, 3, 1), (c, hw * hw, 1)))
        work.append(("resnet50 %d@%d to NCHW" % (c, hw), "transpose", (n, hw, hw, c), (0, 3, 1, 2), (c, hw * hw, 0)))
    work.append(("yolo head 3x85@20", "transpose", (n, 3, 85, 20, 20), (0, 1, 3, 4, 2), None))
    work.append(("head merge 197x12x64", "transpose", (n, 197, 12, 64), (0, 2, 1, 3), None))
    for c, hw in ((32, 112), (64, 112), (128, 56), (256, 28), (512, 14)):
        work.append(("SAME pad %d@%d" % (c, hw), "pad", (n, hw, hw, c), ([0, 0, 0, 0], [0, 1, 1, 0]), None))
    work.append(("flatten 1x1x1024", "flat", (n, 1, 1, 1024), None, None))
    work.append(("flat move 512@28", "flat", (n, 28, 28, 512), None, None))
    lines = ["| layer | op | dtype | kernel | records | us | relu us | op / relu | GB/s | layout.hip us | op / layout.hip |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    for label, op, shape, how, relayout in work:
        for dtype in ("int8", "f16"):
            es = 1 if dtype == "int8" else 2
            code = pkg.SHL_I8 if es == 1 else pkg.SHL_F16
            in_elems = int(np.prod(shape, dtype=np.int64))
            if op == "pad":
                out_elems = int(np.prod([s + b + e for s, b, e in zip(shape, *how)], dtype=np.int64))
            else:
                out_elems = in_elems
            total = (in_elems + out_elems) * es
            block = rng.integers(-128, 128, 1 << 20, dtype=np.int8) if es == 1 else rng.standard_normal(1 << 20).astype(np.float16)
            ins = [dev.alloc(max(in_elems, out_elems) * es) for _ in range(SETS)]
            outs = [dev.alloc(max(in_elems, out_elems) * es) for _ in range(SETS)]
            for b in ins:
                dev.upload(b, np.tile(block, max(in_elems, out_elems) // block.size + 1)[:max(in_elems, out_elems)])
            relu_elems = (in_elems + out_elems) // 2

            def relu_launch(kk):
                i = kk % SETS
                if es == 1:
                    pkg.check(hip.shl_mi355x_relu_i8(ins[i], outs[i], relu_elems, 0.05, 3, 0.04, -2, 0, stream), hip, "relu")
                else:
                    pkg.check(hip.shl_mi355x_relu_f16(ins[i], outs[i], relu_elems, 0, stream), hip, "relu")
            t_relu = timed(relu_launch)
            t_layout = None
            if relayout is not None:
                def layout_launch(kk):
                    i = kk % SETS
                    pkg.check(hip.shl_mi355x_layout_convert(ins[i], outs[i], n, relayout[0], relayout[1], es, relayout[2], stream),
                              hip, "layout_convert")
                t_layout = timed(layout_launch)
            env = "SHL_MI355X_PAD_FORM" if op == "pad" else "SHL_MI355X_TRANSPOSE_FORM"
            forces = ["", "generic"] if op == "pad" else ["", "tile", "rows", "generic"]
            for records in (("equal", "own") if es == 1 else ("-",)):
                out_q = own if records == "own" else in_q
                if op == "transpose":
                    d = pkg.TransposeDesc()
                    d.rank = len(shape)
                    for k in range(len(shape)):
                        d.dim[k], d.perm[k] = shape[k], how[k]
                elif op == "pad":
                    d = pkg.PadDesc()
                    for k in range(4):
                        d.dim[k], d.before[k], d.after[k] = shape[k], how[0][k], how[1][k]
                    d.pad_value = 0.0
                else:
                    d = pkg.MoveDesc()
                d.dtype = code
                d.in_scale, d.in_zp = in_q
                d.out_scale, d.out_zp = out_q

                def launch(kk, what=op):
                    i = kk % SETS
                    if op == "transpose":
                        rc = hip.shl_mi355x_transpose(ins[i], outs[i], C.byref(d), stream)
                    elif op == "pad":
                        rc = hip.shl_mi355x_pad(ins[i], outs[i], C.byref(d), stream)
                    else:
                        rc = hip.shl_mi355x_move(ins[i], outs[i], in_elems, C.byref(d), stream)
                    pkg.check(rc, hip, what)

                def name():
                    if op == "transpose":
                        return hip.shl_mi355x_transpose_kernel_name(ins[0], outs[0], C.byref(d)).decode()
                    if op == "pad":
                        return hip.shl_mi355x_pad_kernel_name(ins[0], outs[0], C.byref(d)).decode()
                    return hip.shl_mi355x_move_kernel_name(ins[0], outs[0], in_elems, C.byref(d)).decode()
                # same answer as the literal form on this data (every set holds the same input)
                os.environ[env] = "generic"
                launch(1, op + " generic")
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                literal = dev.download(outs[1], (out_elems * es,), np.uint8)
                del os.environ[env]
                seen = set()
                for force in forces:
                    if force:
                        os.environ[env] = force
                    kernel = name()
                    # the literal form requantises whatever the records are: timed once per dtype
                    if kernel in seen or (kernel.endswith("generic") and records == "equal" and force):
                        os.environ.pop(env, None)
                        continue
                    seen.add(kernel)
                    launch(0)
                    pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                    if not np.array_equal(dev.download(outs[0], (out_elems * es,), np.uint8), literal):
                        raise SystemExit("move_bench: %s %s %s %s differs from the literal form" % (label, dtype, kernel, records))
                    t = timed(launch)
                    os.environ.pop(env, None)
                    lines.append("| %s | %s | %s | %s | %s | %.2f | %.2f | %.2f | %.0f | %s | %s |" % (
                        label, op, dtype, kernel, records, t * 1e6, t_relu * 1e6, t / t_relu, total / t / 1e9,
                        "%.2f" % (t_layout * 1e6) if t_layout and records != "own" else "-",
                        "%.2f" % (t / t_layout) if t_layout and records != "own" else "-"))
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
