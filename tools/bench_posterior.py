"""Posterior decoding on one MI355X, HBM-resident: cpg_posterior_d over the C2 buffer (46 Mbp)
and the C3 genome (3.1 Gbp), 1 Mi chunks.  Times, with HIP events on the launching stream and
the three variants alternating inside every repetition:
  all     cpg_posterior_d with d_post, d_sign_out and d_loglik
  nopost  cpg_posterior_d with d_post NULL (the path and the log-likelihood only)
  estep   cpg_bw_estep_d over the same bases (65,536-base chunks): the yardstick
A timed window holds `inner` back-to-back calls (so that it is milliseconds long); the figures
are per call: median, min and max over the windows.  write_GBps = 4 B per base over the time
that d_post costs (all).  Prints one JSON line."""
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

SEED = 20251015
CHUNK = 1 << 20


def leg(ctx, dev, seed, nbases, reps, inner, warmup):
    t0 = time.perf_counter()
    packed, _ = D.synth_host(seed, 0, nbases, 16)
    dp = D.to_device(packed, dev)
    del packed
    nch = nbases // CHUNK
    post = torch.empty(nbases + 4, dtype=torch.float32, device=dev)
    sign = torch.empty(D.words32(nbases) + 4, dtype=torch.int32, device=dev)
    ll = torch.empty(max(nch, 1), dtype=torch.float64, device=dev)
    est = torch.empty(_lib.COUNTS_F64_N, dtype=torch.float64, device=dev)
    m = HmmModel.initial()
    ms = m.to_struct()
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0

    def run_all():
        D.posterior(ctx, m, dp, nbases, CHUNK, post_out=post, sign_out=sign, loglik=ll)

    def run_nopost():
        _lib.check(_lib.lib.cpg_posterior_d(ctx.handle, _lib.ptr(ms), D._dp(dp), nbases, CHUNK,
                                            None, D._dp(sign), D._dp(ll), D._stream()))

    def run_estep():
        D.bw_estep(ctx, m, dp, nbases, _lib.TRAIN_CHUNK, out=est)

    variants = {"all": run_all, "nopost": run_nopost, "estep": run_estep}
    res = {k: [] for k in variants}
    for rep in range(warmup + reps):
        marks = {}
        for k, fn in variants.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            marks[k] = (a, b)
        torch.cuda.synchronize()
        ctx.sync()
        if rep >= warmup:
            for k, (a, b) in marks.items():
                res[k].append(a.elapsed_time(b) / inner)
    out = {"bases": nbases, "chunks": nch, "decoded_bases": nch * CHUNK, "reps": reps,
           "inner": inner, "setup_seconds": t_setup, "ms": {}}
    for k, v in res.items():
        out["ms"][k] = {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    nb = nch * CHUNK
    t_all = out["ms"]["all"]["median"] / 1e3
    out["write_GBps"] = 4.0 * nb / t_all / 1e9
    out["bases_per_s"] = {k: (nb if k != "estep" else nbases // _lib.TRAIN_CHUNK * _lib.TRAIN_CHUNK)
                          / (out["ms"][k]["median"] / 1e3) for k in res}
    out["loglik_sum"] = float(ll[:nch].sum().item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2-bases", type=int, default=46_000_000)
    ap.add_argument("--c3-bases", type=int, default=3_100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-c3", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = Context(0)
    out = {"metric": "posterior decoding, HBM-resident, one GPU (1 Mi chunks)", "n_gpus": 1,
           "device": torch.cuda.get_device_name(0),
           "c2": leg(ctx, dev, SEED, args.c2_bases, args.reps, 20, args.warmup)}
    if not args.skip_c3:
        out["c3"] = leg(ctx, dev, SEED + 2, args.c3_bases, max(args.reps // 2, 3), 1, args.warmup)
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
