"""Posterior decoding of a ragged contig batch on one MI355X, HBM-resident: the batch of
tools/bench_contigs.py (log-uniform 150 bp - 50 kbp lengths, bases tiled from a 2^30-base
synthetic genome; default 1M contigs ~ 8.6 Gbases: d_post is 4 B per base).  Times, with HIP
events on the launching stream and the four variants alternating inside every repetition:
  all     cpg_contigs_posterior_d with d_post, d_sign_out and d_loglik
  nopost  cpg_contigs_posterior_d with d_post NULL (the path and the log-likelihoods)
  loglik  cpg_contigs_posterior_d with d_loglik only (the forward pass)
  estep   cpg_contigs_estep_d on the same batch: the yardstick
All with the length schedule (cpg_contigs_order_d, computed once).  Figures per call: median,
min and max over the repetitions.  The path-only form does strictly less per position than
the E-step: its median must not exceed the E-step's by more than the margin = max(10 %, the
E-step's own (max - min) / median in this run); "path_only_vs_estep" holds both medians, the
margin used and the verdict, and the exit status is 1 when the bar is missed.  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("CPG_DEV_PKG"):   # a variant tree from tools/build_variant.sh
    sys.path.insert(0, os.environ["CPG_DEV_PKG"])
from cpgisland_amd import Context, HmmModel, _lib  # noqa: E402
from cpgisland_amd import device as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20251019)
    n = args.contigs
    lens = np.exp(rng.uniform(np.log(150), np.log(50000), n)).astype(np.int64)
    offs, span = D.contig_layout(lens)
    nbases = int(lens.sum())
    t0 = time.perf_counter()
    tile = min(1 << 30, (span + 64 + 1023) // 1024 * 1024)   # (a small --contigs: one tile)
    p1, _ = D.synth_host(20251019, 0, tile, 16)
    wp = tile // 16
    words_p = D.words16(span) + 8
    dp = torch.empty(words_p, dtype=torch.int32, device=dev)
    tp = D.to_device(p1[:wp], dev)
    for i in range(0, words_p, wp):
        k = min(wp, words_p - i)
        dp[i:i + k].copy_(tp[:k])
    del tp, p1
    d_offs = torch.from_numpy(offs).to(dev)
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(dev)
    post = torch.empty((span + 63) // 64 * 64 + 64, dtype=torch.float32, device=dev)
    sign = torch.zeros(D.words32(span) + 8, dtype=torch.int32, device=dev)
    ll = torch.empty(n, dtype=torch.float64, device=dev)
    ecnt = torch.empty(_lib.COUNTS_F64_N, dtype=torch.float64, device=dev)
    ctx = Context(0)
    m = HmmModel.initial()
    order = D.contigs_order(ctx, d_lens, n)
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0

    def posterior(want_post, want_sign):
        D.contigs_posterior(ctx, m, dp, span, d_offs, d_lens, order, n, want_post=want_post,
                            want_sign=want_sign, post_out=post if want_post else None,
                            sign_out=sign if want_sign else None, loglik=ll)

    variants = {"all": lambda: posterior(True, True),
                "nopost": lambda: posterior(False, True),
                "loglik": lambda: posterior(False, False),
                "estep": lambda: D.contigs_estep(ctx, m, dp, span, d_offs, d_lens, order, n,
                                                 out=ecnt)}
    res = {k: [] for k in variants}
    for rep in range(args.warmup + args.reps):
        marks = {}
        for k, fn in variants.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            marks[k] = (a, b)
        torch.cuda.synchronize()
        ctx.sync()
        if rep >= args.warmup:
            for k, (a, b) in marks.items():
                res[k].append(a.elapsed_time(b))
    ms = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in res.items()}
    e = ms["estep"]
    spread = (e["max"] - e["min"]) / e["median"]
    margin = max(0.10, spread)
    ok = ms["nopost"]["median"] <= e["median"] * (1.0 + margin)
    out = {"metric": "posterior decoding, ragged contig batch, HBM-resident, one GPU",
           "n_gpus": 1, "device": torch.cuda.get_device_name(0), "contigs": n, "bases": nbases,
           "span": span, "reps": args.reps, "warmup": args.warmup, "setup_seconds": t_setup,
           "ms": ms,
           "bases_per_s": {k: nbases / (v["median"] / 1e3) for k, v in ms.items()},
           "write_GBps": 4.0 * nbases / (ms["all"]["median"] / 1e3) / 1e9,
           "ratio_to_estep": {k: v["median"] / e["median"] for k, v in ms.items()},
           "path_only_vs_estep": {"nopost_median_ms": ms["nopost"]["median"],
                                  "estep_median_ms": e["median"], "estep_spread": spread,
                                  "margin": margin, "within_bar": bool(ok)},
           "loglik_sum": float(ll.sum().item()),
           "data": "log-uniform 150-50000 bp lengths; bases tiled from a synthetic genome"}
    print(json.dumps(out), flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
