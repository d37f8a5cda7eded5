#!/usr/bin/env python3
"""The fused attention core (shl_mi355x_attention) against the launches it replaces, through the C-ABI (no torch).

    python tools/attention_bench.py [--reps 4] [--only NAME[,NAME]] [--out FILE.md]
Per shape and dtype two hipGraphs are captured, each holding `reps` units of work that rotate over three buffer sets (so that
a unit does not find its operands in the last-level cache):
  * fused     one launch per unit: what a session's STEP_ATTENTION enqueues;
  * unfused   the launches the same session captures with SHL_MI355X_ATTENTION=0: shl_mi355x_matmul (q k^T), shl_mi355x_mul,
              shl_mi355x_softmax, shl_mi355x_matmul (p v) -- the parent commit's kernels, which this change leaves as they
              were -- with the scores and the probabilities through HBM.
Each graph is replayed 20 times between two HIP events; the figure is the median of five such windows per unit, "spread" the
range of the five windows over their median.  Before timing, the fused output is compared with the unfused one bit for bit.
A shape whose products the matmul form rule gives to the chain form has no fused kernel: its row says so and times the unfused
launches only.  Prints a markdown table with the launch counts.

Shapes: ViT-B/16 (12 heads, 197 tokens, d 64) at batch 1 and 8, DeiT-tiny (3 heads), a MobileViT stage (64 tokens, 4 heads over
4 patch positions, d 60 -- and the same at d 64), 8 heads of 64 on 384, 512 and 640 tokens (where the default rule's bound on
the keys comes from), a DETR encoder layer (8 heads, 850 tokens, d 32).
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
SHAPES = [
    # name, batches (images x heads), S, T, d, dv
    ("vit_b16_b1", 12, 197, 197, 64, 64),
    ("deit_tiny_b1", 3, 197, 197, 64, 64),
    ("mobilevit_64tok_d60", 16, 64, 64, 60, 60),
    ("mobilevit_64tok_d64", 16, 64, 64, 64, 64),
    ("enc_384tok_d64", 8, 384, 384, 64, 64),
    ("enc_512tok_d64", 8, 512, 512, 64, 64),
    ("enc_640tok_d64", 8, 640, 640, 64, 64),
    ("detr_850tok_d32", 8, 850, 850, 32, 32),
    ("vit_b16_b8", 96, 197, 197, 64, 64),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import attention_cases as ac
    import cases
    pkg = cases.pkg
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("attention_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
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
            raise SystemExit("attention_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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

    head = ["shape", "batches x S x T x d", "dtype", "launches fused / unfused", "unfused us", "spread", "fused us", "spread", "fused / unfused"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    only = set(filter(None, a.only.split(",")))
    for name, batches, s, t, d, dv in SHAPES:
        if only and name not in only:
            continue
        for dtype in ("int8", "f16"):
            made = []
            ac._add(made, name, dtype, s=s, t=t, d=d, dv=dv, batches=batches, regime="conv")
            c = made[0]
            es = c["q"].itemsize
            code = pkg.SHL_I8 if dtype == "int8" else pkg.SHL_F16
            bufs = []
            for _ in range(SETS):
                b = {key: dev.alloc(c[key].nbytes) for key in ("q", "k", "v", "c")}
                for key in ("q", "k", "v", "c"):
                    dev.upload(b[key], c[key])
                for key in ("s", "x", "p"):
                    b[key] = dev.alloc(batches * s * t * es)
                for key in ("chain", "fused"):
                    b[key] = dev.alloc(batches * s * dv * es)
                bufs.append(b)
            desc = ac.desc(c)
            qk, mul, pv = ac.unfused_descs(c)

            def unfused(kk):
                b = bufs[kk % SETS]
                pkg.check(hip.shl_mi355x_matmul(b["q"], b["k"], b["s"], C.byref(qk), stream), hip, "matmul (q k^T)")
                pkg.check(hip.shl_mi355x_mul(b["s"], b["c"], b["x"], C.byref(mul), stream), hip, "mul")
                pkg.check(hip.shl_mi355x_softmax(b["x"], b["p"], code, batches * s, t, 1, c["sc_q"][0], c["sc_q"][1], c["p_q"][0],
                                                 c["p_q"][1], stream), hip, "softmax")
                pkg.check(hip.shl_mi355x_matmul(b["p"], b["v"], b["chain"], C.byref(pv), stream), hip, "matmul (p v)")

            def fused(kk):
                b = bufs[kk % SETS]
                pkg.check(hip.shl_mi355x_attention(b["q"], b["k"], b["v"], b["fused"], C.byref(desc), stream), hip, "attention")

            def fetch(p):
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                return dev.download(p, (batches * s * dv,), c["q"].dtype).view(np.uint8 if es == 1 else np.uint16)
            b0 = bufs[0]
            has_kernel = hip.shl_mi355x_attention_kernel_name(b0["q"], b0["k"], b0["v"], b0["fused"], C.byref(desc)) != b""
            forms = "%s, %s" % (hip.shl_mi355x_matmul_kernel_name(b0["q"], b0["k"], b0["s"], C.byref(qk)).decode().replace("matmul_", ""),
                                hip.shl_mi355x_matmul_kernel_name(b0["p"], b0["v"], b0["chain"], C.byref(pv)).decode().replace("matmul_", ""))
            t_un, sp_un = timed(unfused, a.reps)
            cells = [name, "%d x %d x %d x %d" % (batches, s, t, d), dtype]
            if has_kernel:
                unfused(0)
                want = fetch(b0["chain"])
                fused(0)
                if not np.array_equal(fetch(b0["fused"]), want):
                    raise SystemExit("attention_bench: %s %s: the fused launch differs from the unfused launches" % (name, dtype))
                t_f, sp_f = timed(fused, a.reps)
                cells += ["1 / 4", "%.2f" % (t_un * 1e6), "%.0f %%" % (100 * sp_un), "%.2f" % (t_f * 1e6), "%.0f %%" % (100 * sp_f),
                          "%.2f" % (t_f / t_un)]
            else:
                cells += ["- / 4", "%.2f" % (t_un * 1e6), "%.0f %%" % (100 * sp_un), "no kernel (%s)" % forms, "-", "-"]
            row = "| " + " | ".join(cells) + " |"
            lines.append(row)
            print(row, flush=True)
            for b in bufs:
                for p in b.values():
                    dev.free(p)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
