#!/usr/bin/env python3
"""The matmul kernels -- both forms -- against the pointwise convolution plan of equal M, K, N, through the C-ABI (no torch).

    python tools/matmul_bench.py [--seq 49,197,256] [--heads 12] [--reps 8] [--small 1,2,4,8,16,32] [--out FILE.md]
Times, in int8 and binary16:
  * QK^T of an attention block: heads x S x 64 x S (trans_b), and P V: heads x S x S x 64,
  * the linear layers of a ViT-B encoder as matmul against a constant: S x 768 x 768 and S x 768 x 3072,
  * the same 768 x 768 layer at a few rows (--small): the decode shape M = 1 and the crossover of the default rule,
each forced to the chain form and to the mfma form (SHL_MI355X_MATMUL_FORM), with the form the default rule picks named.
Each `reps` launches captured in one hipGraph (rotating over three buffer sets, so that a launch does not find its operands in
the last-level cache), the graph replayed 20 times between two HIP events, median of five such windows.  The yardstick, timed
the same way in the same process: the project's own GEMM, a 1x1 convolution plan (selection rules, no tuning) over `batches`
images of 1 x M pixels with K input and N output channels.  Prints a markdown table.  Before timing, the int8 mfma output is
compared with the chain's on the device's own data (power-of-two scales inside the plan-time proof: bit for bit) and the
binary16 one within 1e-3.
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
ENV = "SHL_MI355X_MATMUL_FORM"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", default="49,197,256")
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--small", default="1,2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cases
    import deconv_cases as dc
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("matmul_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()

    def timed(enqueue, reps):
        """enqueue(k): the k-th launch on `stream`; (seconds per launch, spread of the windows as a fraction)"""
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for k in range(reps):
            enqueue(k)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("matmul_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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
        return windows[2] * 1e-3 / (20 * reps), (windows[-1] - windows[0]) / windows[2]

    work = []  # (label, batches, m, k, n, trans_b, mat1 shared by the batches)
    for s in [int(v) for v in a.seq.split(",")]:
        work.append(("QK^T %dx%dx64x%d" % (a.heads, s, s), a.heads, s, 64, s, True, False))
        work.append(("P V %dx%dx%dx64" % (a.heads, s, s), a.heads, s, s, 64, False, False))
        work.append(("linear %dx768x768" % s, 1, s, 768, 768, False, True))
        work.append(("linear %dx768x3072" % s, 1, s, 768, 3072, False, True))
    for m in [int(v) for v in a.small.split(",") if v]:
        work.append(("rows %dx768x768" % m, 1, m, 768, 768, False, True))
    lines = ["| problem | dtype | default | chain us | mfma us | chain / mfma | 1x1 plan | 1x1 us | mfma / 1x1 | mfma TMAC/s | spread |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    os.environ["SHL_MI355X_TUNE"] = "0"  # the yardstick by the selection rules: the same kernel on every box
    rng = np.random.default_rng(1)
    for label, nb, m, k, n, tb, _ in work:
        for dtype in ("int8", "f16"):
            es = 1 if dtype == "int8" else 2
            a_shape = (nb, m, k) if nb > 1 else (m, k)
            b_shape = ((nb,) if nb > 1 else ()) + ((n, k) if tb else (k, n))
            if es == 1:
                xa, xb = rng.integers(-128, 128, a_shape, dtype=np.int8), rng.integers(-128, 128, b_shape, dtype=np.int8)
            else:
                xa, xb = rng.standard_normal(a_shape).astype(np.float16), (0.1 * rng.standard_normal(b_shape)).astype(np.float16)
            out_elems = nb * m * n
            d = pkg.matmul_desc(pkg.SHL_I8 if es == 1 else pkg.SHL_F16, a_shape, b_shape, False, tb, (2.0 ** -4, 3), (2.0 ** -7, 0),
                                (float(np.float32(2.0 ** -11 * 74 * 74 * np.sqrt(k) / 40)), -5))
            bufs_a, bufs_b = [dev.alloc(xa.nbytes) for _ in range(SETS)], [dev.alloc(xb.nbytes) for _ in range(SETS)]
            outs = [dev.alloc(out_elems * es) for _ in range(SETS)]
            for p in bufs_a:
                dev.upload(p, xa)
            for p in bufs_b:
                dev.upload(p, xb)

            def launch(kk):
                i = kk % SETS
                pkg.check(hip.shl_mi355x_matmul(bufs_a[i], bufs_b[i], outs[i], C.byref(d), stream), hip, "matmul")
            default = hip.shl_mi355x_matmul_kernel_name(bufs_a[0], bufs_b[0], outs[0], C.byref(d)).decode()
            t, got = {}, {}
            for form in ("chain", "mfma"):
                os.environ[ENV] = form
                ran = hip.shl_mi355x_matmul_kernel_name(bufs_a[0], bufs_b[0], outs[0], C.byref(d)).decode()
                if ran != "matmul_" + form:
                    raise SystemExit("matmul_bench: %s %s: asked for %s, the rule gives %s" % (label, dtype, form, ran))
                launch(0)
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                got[form] = dev.download(outs[0], (out_elems,), np.int8 if es == 1 else np.float16)
                t[form] = timed(launch, a.reps)
                del os.environ[ENV]
            if es == 1:
                if hip.shl_mi355x_matmul_is_exact(C.byref(d)) and not np.array_equal(got["chain"], got["mfma"]):
                    raise SystemExit("matmul_bench: %s int8: the mfma form differs from the chain inside the proof" % label)
                worst = int(np.abs(got["chain"].astype(np.int32) - got["mfma"].astype(np.int32)).max())
                if worst > 1:
                    raise SystemExit("matmul_bench: %s int8: the mfma form is %d LSB from the chain" % (label, worst))
            else:
                g, w = got["mfma"].astype(np.float64), got["chain"].astype(np.float64)
                if not np.all(np.abs(g - w) <= 2e-3 * np.maximum(np.abs(w), 0.05)):  # (signed sums: cancellation allowed for)
                    raise SystemExit("matmul_bench: %s binary16: the mfma form is off the chain" % label)
            # the yardstick: a 1x1 convolution over nb images of 1 x m pixels, k -> n channels
            case = dc.make("matmul_yardstick_%s_%s" % (label, dtype), dtype=dtype, regime="general", n=nb, h=1, w=m, c=k, co=n, k=(1, 1),
                           stride=(1, 1), pad=(0,) * 4, normal=True)
            mult, bias = dc.tables(case)
            plan = C.c_void_p()
            desc = dc.deconv_desc(case)
            kern = np.ascontiguousarray(case["kernel"])
            pkg.check(hip.shl_mi355x_conv_plan_create(C.byref(desc), kern.ctypes.data, mult.ctypes.data if es == 1 else None,
                                                      bias.ctypes.data, None, C.byref(plan)), hip, "conv_plan_create")
            pw_name = hip.shl_mi355x_conv_plan_kernel_name(plan).decode()
            t_pw, _ = timed(lambda kk: pkg.check(hip.shl_mi355x_conv_forward(plan, bufs_a[kk % SETS], outs[kk % SETS], nb, stream), hip, "forward"),
                            a.reps)
            hip.shl_mi355x_conv_plan_destroy(plan)
            macs = nb * m * n * k
            (t_c, sp_c), (t_m, sp_m) = t["chain"], t["mfma"]
            lines.append("| %s | %s | %s | %.1f | %.1f | %.2f | %s | %.1f | %.2f | %.2f | %.0f %% / %.0f %% |" % (
                label, dtype, default.replace("matmul_", ""), t_c * 1e6, t_m * 1e6, t_c / t_m, pw_name, t_pw * 1e6, t_m / t_pw,
                macs / t_m / 1e12, 100 * sp_c, 100 * sp_m))
            print(lines[-1], flush=True)
            for p in bufs_a + bufs_b + outs:
                dev.free(p)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
