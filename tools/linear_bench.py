#!/usr/bin/env python3
"""The broadcasting add and the fused linear layer (matmul + add of a constant bias), through the C-ABI (no torch).

    python tools/linear_bench.py [--seq 17,197] [--reps 8] [--base-lib OTHER/libshl_mi355x.so] [--out FILE.md]
Two tables, int8 and binary16:
  * the broadcasting add's forms -- the one the rule picks (add_vec for [.., N] + [N], add_row for NCHW [1,C,1,1]) and
    add_generic (SHL_MI355X_ADD_FORM=generic) -- against the project's streaming same-shape add (shl_mi355x_add) on the same
    number of output bytes: [1,197,768] + [768], [8,197,768] + [768], NCHW [1,64,56,56] + [1,64,1,1];
  * the linear layers S x 768 x 768, S x 768 x 3072 and S x 384 x 1536 in the matmul form the rule picks: shl_mi355x_matmul
    alone, matmul followed by shl_mi355x_add_bcast (two launches, the intermediate through HBM) and shl_mi355x_matmul_bias (one
    launch); with --base-lib also the matmul of another build of the library (the parent commit's), in the same process.
Each `reps` launches captured in one hipGraph (rotating over three buffer sets, so that a launch does not find its operands in
the last-level cache), the graph replayed 20 times between two HIP events, median of five such windows; "spread" is the range
of the five windows over their median.  Before timing, the add's forms are compared with each other bit for bit, and the fused
launch with the pair bit for bit.  Prints two markdown tables.
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
    ap.add_argument("--seq", default="17,197")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--base-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import add_bcast_cases
    import cases
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("linear_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    base = None
    if a.base_lib:
        base = C.CDLL(os.path.abspath(a.base_lib), mode=C.RTLD_LOCAL)
        vp = C.c_void_p
        base.shl_mi355x_matmul.restype, base.shl_mi355x_matmul.argtypes = C.c_int, [vp, vp, vp, C.POINTER(pkg.MatmulDesc), vp]
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()

    def timed(enqueue, reps):
        """enqueue(k): the k-th unit of work on `stream`; (seconds per unit, range of the windows over their median)"""
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for k in range(reps):
            enqueue(k)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("linear_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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

    rng = np.random.default_rng(1)
    text = []

    def data(shape, es, scale=1.0):
        if es == 1:
            return rng.integers(-128, 128, shape, dtype=np.int8)
        return (scale * rng.standard_normal(shape)).astype(np.float16)

    def fetch(p, elems, es):
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
        return dev.download(p, (elems,), np.int8 if es == 1 else np.float16).view(np.uint8 if es == 1 else np.uint16)

    # ---- the broadcasting add against the same-shape add ------------------------------------------------------------------
    lines = ["| problem | dtype | form | same-shape add us | spread | form us | spread | form / add | generic us | generic / add |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    q = ((2.0 ** -4, -5), (2.0 ** -5, 3), (2.0 ** -3, 9))
    for label, a_shape, b_shape in (("[1,197,768]+[768]", (1, 197, 768), (768,)), ("[8,197,768]+[768]", (8, 197, 768), (768,)),
                                    ("NCHW [1,64,56,56]+[1,64,1,1]", (1, 64, 56, 56), (1, 64, 1, 1))):
        for dtype in ("int8", "f16"):
            es = 1 if dtype == "int8" else 2
            xa, xb, xs = data(a_shape, es), data(b_shape, es), data(a_shape, es)
            count = xa.size
            desc = add_bcast_cases.add_desc(dict(dtype=dtype, in_q=q[0], in1_q=q[1], out_q=q[2]), a_shape, b_shape)
            A = [dev.alloc(xa.nbytes) for _ in range(SETS)]
            S = [dev.alloc(xs.nbytes) for _ in range(SETS)]
            B = [dev.alloc(max(xb.nbytes, 16)) for _ in range(SETS)]
            O = [dev.alloc(xa.nbytes) for _ in range(SETS)]
            for i in range(SETS):
                dev.upload(A[i], xa), dev.upload(S[i], xs), dev.upload(B[i], xb)
            code = pkg.SHL_I8 if es == 1 else pkg.SHL_F16

            def same(kk):
                i = kk % SETS
                pkg.check(hip.shl_mi355x_add(A[i], S[i], O[i], count, code, q[0][0], q[0][1], q[1][0], q[1][1], q[2][0], q[2][1], stream),
                          hip, "add")

            def bcast(kk):
                i = kk % SETS
                pkg.check(hip.shl_mi355x_add_bcast(A[i], B[i], O[i], C.byref(desc), stream), hip, "add_bcast")
            os.environ.pop("SHL_MI355X_ADD_FORM", None)
            form = hip.shl_mi355x_add_bcast_kernel_name(C.byref(desc), A[0], B[0], O[0]).decode()
            bcast(0)
            got = fetch(O[0], count, es)
            t_same, sp_same = timed(same, a.reps)
            t_form, sp_form = timed(bcast, a.reps)
            os.environ["SHL_MI355X_ADD_FORM"] = "generic"
            bcast(0)
            if not np.array_equal(fetch(O[0], count, es), got):
                raise SystemExit("linear_bench: %s %s: %s differs from add_generic" % (label, dtype, form))
            t_gen, _ = timed(bcast, a.reps)
            del os.environ["SHL_MI355X_ADD_FORM"]
            lines.append("| %s | %s | %s | %.2f | %.0f %% | %.2f | %.0f %% | %.2f | %.2f | %.2f |" % (
                label, dtype, form, t_same * 1e6, 100 * sp_same, t_form * 1e6, 100 * sp_form, t_form / t_same, t_gen * 1e6, t_gen / t_same))
            print(lines[-1], flush=True)
            for p in A + S + B + O:
                dev.free(p)
    text += lines + [""]

    # ---- the fused linear layer ---------------------------------------------------------------------------------------------
    head = ["problem", "dtype", "form"] + (["parent matmul us", "spread"] if base else []) + [
        "matmul us", "spread", "matmul + add_bcast us", "fused us", "spread", "fused / pair", "fused / matmul"] + (
        ["fused / parent matmul"] if base else [])
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    work = []
    for s in [int(v) for v in a.seq.split(",")]:
        work += [(s, 768, 768), (s, 768, 3072), (s, 384, 1536)]
    for m, k, n in work:
        for dtype in ("int8", "f16"):
            es = 1 if dtype == "int8" else 2
            xa, xb, xc = data((m, k), es), data((k, n), es, 0.1), data((n,), es)
            spread = float(np.float32(2.0 ** -11 * 74 * 74 * np.sqrt(k) / 40))
            rec_mid, rec_bias, rec_out = (spread, -5), (spread / 2, 7), (spread * 1.5, 3)
            code = pkg.SHL_I8 if es == 1 else pkg.SHL_F16
            d_mid = pkg.matmul_desc(code, (m, k), (k, n), False, False, (2.0 ** -4, 3), (2.0 ** -7, 0), rec_mid)
            d_out = pkg.matmul_desc(code, (m, k), (k, n), False, False, (2.0 ** -4, 3), (2.0 ** -7, 0), rec_out)
            add = add_bcast_cases.add_desc(dict(dtype=dtype, in_q=rec_mid, in1_q=rec_bias, out_q=rec_out), (m, n), (n,))
            A, B = [dev.alloc(xa.nbytes) for _ in range(SETS)], [dev.alloc(xb.nbytes) for _ in range(SETS)]
            Cb = [dev.alloc(xc.nbytes) for _ in range(SETS)]
            M, O = [dev.alloc(m * n * es) for _ in range(SETS)], [dev.alloc(m * n * es) for _ in range(SETS)]
            for i in range(SETS):
                dev.upload(A[i], xa), dev.upload(B[i], xb), dev.upload(Cb[i], xc)

            def alone(kk, lib=hip):
                i = kk % SETS
                pkg.check(lib.shl_mi355x_matmul(A[i], B[i], M[i], C.byref(d_mid), stream), hip, "matmul")

            def pair(kk):
                i = kk % SETS
                alone(kk)
                pkg.check(hip.shl_mi355x_add_bcast(M[i], Cb[i], O[i], C.byref(add), stream), hip, "add_bcast")

            def fused(kk):
                i = kk % SETS
                pkg.check(hip.shl_mi355x_matmul_bias(A[i], B[i], Cb[i], O[i], C.byref(d_out), rec_bias[0], rec_bias[1], rec_mid[0],
                                                     rec_mid[1], 0, stream), hip, "matmul_bias")
            form = hip.shl_mi355x_matmul_bias_kernel_name(A[0], B[0], Cb[0], O[0], C.byref(d_out)).decode()
            pair(0)
            want = fetch(O[0], m * n, es)
            fused(0)
            if not np.array_equal(fetch(O[0], m * n, es), want):
                raise SystemExit("linear_bench: %dx%dx%d %s: the fused launch differs from matmul followed by add_bcast" % (m, k, n, dtype))
            (t_mm, sp_mm), (t_pair, _), (t_fused, sp_fused) = timed(alone, a.reps), timed(pair, a.reps), timed(fused, a.reps)
            cells = ["linear %dx%dx%d" % (m, k, n), dtype, form.replace("matmul_", "")]
            if base:
                t_base, sp_base = timed(lambda kk: alone(kk, base), a.reps)
                cells += ["%.2f" % (t_base * 1e6), "%.0f %%" % (100 * sp_base)]
            cells += ["%.2f" % (t_mm * 1e6), "%.0f %%" % (100 * sp_mm), "%.2f" % (t_pair * 1e6), "%.2f" % (t_fused * 1e6),
                      "%.0f %%" % (100 * sp_fused), "%.2f" % (t_fused / t_pair), "%.2f" % (t_fused / t_mm)]
            if base:
                cells.append("%.2f" % (t_fused / t_base))
            row = "| " + " | ".join(cells) + " |"
            lines.append(row)
            print(row, flush=True)
            for p in A + B + Cb + M + O:
                dev.free(p)
    text += lines
    text = "\n".join(text) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
