"""Posterior decoding of ragged contig batches on the GPU (cpg_contigs_posterior_d,
cpg_contigs_island_confidence_d) against the fp64 reference of tests/test_posterior_ref.py
applied per contig.  One batch: the edge lengths of tests/test_gpu_contigs.py, 48 log-uniform
lengths of 150 - 8000 bases, 20000 and 66000 (more than one 64-block, more than one wave's
worth of contigs, a contig past 65,536), 17 bases of gap, shuffled; bases from the synthetic
genome at seed 20251015; models from oracle/families.py.

Tolerances (those of tests/test_gpu_posterior.py): d_post within 1 float32 ulp of
float32(reference) (both sides carry fp64 error far below 2^-24, so only a value next to a
rounding boundary can differ, by one ulp; below 2^-126 either 0 or the denormal); d_loglik 1e-9
relative (the E-step's); a float32 mean of float32 values 2^-23 relative."""
import functools

import numpy as np
import pytest

from oracle import coracle as co
from oracle import families as fam
from oracle import pyref as pr

from test_gpu_contigs import EDGE
from test_gpu_posterior import assert_post_close
from test_posterior_ref import SEED, posterior_ref

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A          # sign words the kernel must leave alone
FAMILIES = ["initial", "random_norm0", "pi_tiny", "pow2"]
ORDERED = "random_norm0"   # the family that runs with the length schedule


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _batch():
    from cpgisland_amd import device as D
    rng = np.random.default_rng(11)
    lens = np.exp(rng.uniform(np.log(150), np.log(8000), 48)).astype(np.int64)
    lens = np.concatenate([EDGE, lens, [20000, 66000]]).astype(np.int64)
    rng.shuffle(lens)
    offs, span = D.contig_layout(lens, gap=17)
    packed, _ = D.synth_host(SEED, 0, span + 64)
    obs = pr.unpack(packed, span + 64)
    n = len(lens)
    cap = (span + 63) // 64 * 64                 # floats of d_post
    own = np.zeros(cap, bool)                     # a contig's bases
    pad = np.zeros(cap, bool)                     # past a contig's end, inside its last block
    wown = np.zeros(cap // 32, bool)              # sign words of the contigs' blocks
    for c in range(n):
        o, L = int(offs[c]), int(lens[c])
        e = o + (L + 63) // 64 * 64
        own[o:o + L] = True
        pad[o + L:e] = True
        wown[o // 32:e // 32] = True
    for a in (lens, offs, obs, own, pad, wown):
        a.setflags(write=False)
    return {"lens": lens, "offs": offs, "span": span, "packed": packed, "obs": obs, "n": n,
            "cap": cap, "own": own, "pad": pad, "wown": wown}


def test_batch_is_the_one_described():
    b = _batch()
    assert (b["n"], int(b["lens"].sum()), b["span"]) == (66, 175260, 178793)


_DEV = {}


def _dev_batch(dev):
    import torch
    from cpgisland_amd import device as D
    if "b" not in _DEV:
        b = _batch()
        _DEV["b"] = {
            "packed": D.to_device(np.concatenate([b["packed"], np.zeros(8, np.uint32)]), dev),
            "offs": torch.from_numpy(b["offs"].copy()).to(dev),
            "lens": torch.from_numpy(b["lens"].astype(np.int32)).to(dev)}
    return _DEV["b"]


def _model(name):
    if name == "zero_pi":                        # pi of both live states of base 0 (A) at 0
        m = fam.family("initial").copy()
        m[[0, 4]] = 0.0
        return m
    return fam.family(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(posterior per base of the span, fp64, 0 outside the contigs; log-likelihood per contig)"""
    b = _batch()
    m = _model(name)
    ref = np.zeros(b["cap"])
    ll = np.zeros(b["n"])
    for c in range(b["n"]):
        o, L = int(b["offs"][c]), int(b["lens"][c])
        ref[o:o + L], ll[c] = posterior_ref(m, b["obs"][o:o + L])
    ref.setflags(write=False)
    ll.setflags(write=False)
    return ref, ll


def _run(ctx, dev, model, order=False, want_post=True, want_sign=True, want_ll=True,
         post_offset=0, offs=None, lens=None, nbases=None):
    """cpg_contigs_posterior_d on the batch, outputs behind sentinels; returns the status code
    and (post float32 | None, sign uint32 words | None, loglik | None)."""
    import torch
    from cpgisland_amd import _lib
    from cpgisland_amd import device as D
    b, d = _batch(), _dev_batch(dev)
    d_offs = d["offs"] if offs is None else offs
    d_lens = d["lens"] if lens is None else lens
    n = d_lens.shape[0]
    nbases = b["span"] if nbases is None else nbases
    cap = (nbases + 63) // 64 * 64
    post = torch.full((cap + 64,), float("nan"), dtype=torch.float32, device=dev)
    sign = torch.full((cap // 32 + 4,), SENT, dtype=torch.int32, device=dev)
    ll = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    d_order = D.contigs_order(ctx, d_lens, n) if order else None
    m = np.ascontiguousarray(model, np.float64)
    rc = _lib.lib.cpg_contigs_posterior_d(
        ctx.handle, _lib.ptr(m), D._dp(d["packed"]), nbases, D._dp(d_offs), D._dp(d_lens),
        D._opt(d_order), n, D._dp(post[post_offset:]) if want_post else None,
        D._dp(sign) if want_sign else None, D._dp(ll) if want_ll else None, D._stream())
    torch.cuda.synchronize()
    return rc, (post.cpu().numpy() if want_post else None,
                sign.cpu().numpy().view(np.uint32) if want_sign else None,
                ll.cpu().numpy() if want_ll else None)


def _run_ok(ctx, dev, model, **kw):
    from cpgisland_amd import _lib
    rc, out = _run(ctx, dev, model, **kw)
    _lib.check(rc)
    ctx.sync()
    return out


_OUT = {}


def _outputs(ctx, dev, name):
    """All three outputs of the family, run once (with the length schedule for ORDERED)."""
    if name not in _OUT:
        _OUT[name] = _run_ok(ctx, dev, _model(name), order=name == ORDERED)
    return _OUT[name]


def _bits(sign):
    b = _batch()
    return pr.unpack_bits(sign[: b["cap"] // 32], b["cap"])


def _check_layout(post, sign):
    """What lies outside the contigs: padding floats 0, padding bits 0, the rest untouched."""
    b = _batch()
    cap = b["cap"]
    assert np.all(post[:cap][b["pad"]] == 0.0)
    assert np.isnan(post[:cap][~(b["own"] | b["pad"])]).all() and np.isnan(post[cap:]).all()
    assert not _bits(sign)[b["pad"]].any()
    assert np.all(sign[: cap // 32][~b["wown"]] == SENT) and np.all(sign[cap // 32:] == SENT)


@pytest.mark.parametrize("name", FAMILIES)
def test_parity(gpu_ctx, dev, name):
    b = _batch()
    post, sign, ll = _outputs(gpu_ctx, dev, name)
    ref, rll = _reference(name)
    own = b["own"]
    print(name, "ref min", ref[own].min(), "near 0.5:", int((np.abs(ref[own] - 0.5) < 1e-6).sum()),
          "loglik max rel", np.max(np.abs(ll - rll) / np.abs(rll)))
    assert_post_close(post[: b["cap"]][own], ref[own])
    _check_layout(post, sign)
    clear = own & (np.abs(ref - 0.5) >= 1e-6)
    assert (own & ~clear).sum() <= 1e-3 * own.sum()
    assert np.array_equal(_bits(sign)[clear], (ref > 0.5)[clear].astype(np.uint8))
    assert np.all(np.abs(ll - rll) <= 1e-9 * np.abs(rll)), (ll, rll)
    if name == "pi_tiny":                        # the flush to 0 is exercised
        assert ref[own].min() < 1e-45


def _same_bits(x, y):
    return (np.array_equal(x[0].view(np.int32), y[0].view(np.int32)) and
            np.array_equal(x[1], y[1]) and np.array_equal(x[2].view(np.int64), y[2].view(np.int64)))


def test_schedule_independent_and_reproducible(gpu_ctx, dev):
    m = _model("initial")
    plain = _outputs(gpu_ctx, dev, "initial")    # batch order
    assert _same_bits(plain, _run_ok(gpu_ctx, dev, m, order=True))
    assert _same_bits(plain, _run_ok(gpu_ctx, dev, m))


def test_output_subsets(gpu_ctx, dev):
    from cpgisland_amd import _lib
    m = _model("initial")
    _, sign, ll = _outputs(gpu_ctx, dev, "initial")
    _, s2, l2 = _run_ok(gpu_ctx, dev, m, want_post=False)
    assert np.array_equal(s2, sign) and np.array_equal(l2.view(np.int64), ll.view(np.int64))
    _, _, l3 = _run_ok(gpu_ctx, dev, m, want_post=False, want_sign=False)
    assert np.array_equal(l3.view(np.int64), ll.view(np.int64))
    rc, _ = _run(gpu_ctx, dev, m, want_post=False, want_sign=False, want_ll=False)
    assert rc == _lib.CPG_OK
    gpu_ctx.sync()


def test_device_wrapper(gpu_ctx, dev):
    """D.contigs_posterior: the same bits, None for what is not wanted."""
    import torch
    from cpgisland_amd import HmmModel
    from cpgisland_amd import device as D
    b, d = _batch(), _dev_batch(dev)
    post, sign, ll = _outputs(gpu_ctx, dev, "initial")
    m = HmmModel.from_struct(_model("initial"))
    p, s, l = D.contigs_posterior(gpu_ctx, m, d["packed"], b["span"], d["offs"], d["lens"], None,
                                  b["n"])
    torch.cuda.synchronize()
    gpu_ctx.sync()
    own = b["own"]
    assert np.array_equal(p.cpu().numpy()[: b["cap"]][own].view(np.int32),
                          post[: b["cap"]][own].view(np.int32))
    assert np.array_equal(_bits(s.cpu().numpy().view(np.uint32))[own], _bits(sign)[own])
    assert np.array_equal(l.cpu().numpy().view(np.int64), ll.view(np.int64))
    p, s, l = D.contigs_posterior(gpu_ctx, m, d["packed"], b["span"], d["offs"], d["lens"], None,
                                  b["n"], want_post=False, want_sign=False)
    torch.cuda.synchronize()
    gpu_ctx.sync()
    assert p is None and s is None
    assert np.array_equal(l.cpu().numpy().view(np.int64), ll.view(np.int64))


def test_zero_probability_contigs(gpu_ctx, dev):
    b = _batch()
    post, sign, ll = _run_ok(gpu_ctx, dev, _model("zero_pi"))
    ref, rll = _reference("zero_pi")
    _check_layout(post, sign)
    assert not np.isnan(post[: b["cap"]][b["own"]]).any()
    bits = _bits(sign)
    dead = 0
    for c in range(b["n"]):
        o, L = int(b["offs"][c]), int(b["lens"][c])
        if b["obs"][o] == 0:
            dead += 1
            assert ll[c] == -np.inf and not post[o:o + L].any()
            assert not sign[o // 32:(o + L + 63) // 64 * 2].any()
        else:
            assert_post_close(post[o:o + L], ref[o:o + L])
            assert abs(ll[c] - rll[c]) <= 1e-9 * abs(rll[c])
            sl = slice(o, o + L)
            clear = np.abs(ref[sl] - 0.5) >= 1e-6
            assert np.array_equal(bits[sl][clear], (ref[sl] > 0.5)[clear].astype(np.uint8))
    assert 0 < dead < b["n"]


def _islands_of(ctx, dev, sign):
    import torch
    from cpgisland_amd import device as D
    b, d = _batch(), _dev_batch(dev)
    ds = torch.from_numpy(sign.view(np.int32).copy()).to(dev)
    out, cnt = D.contigs_islands(ctx, d["packed"], ds, b["span"], d["offs"], d["lens"], None,
                                 b["n"], cap=4096)
    torch.cuda.synchronize()
    ctx.sync()
    return out, cnt


def test_islands_and_confidence(gpu_ctx, dev):
    import torch
    from cpgisland_amd import device as D
    b, d = _batch(), _dev_batch(dev)
    post, sign, _ = _outputs(gpu_ctx, dev, "initial")
    ref, _ = _reference("initial")
    out, cnt = _islands_of(gpu_ctx, dev, sign)
    recs = D.islands_to_numpy(out, cnt)
    want = []
    for c in range(b["n"]):
        o, L = int(b["offs"][c]), int(b["lens"][c])
        states = b["obs"][o:o + L].astype(np.int32) + np.where(ref[o:o + L] > 0.5, 0, 4)
        r = co.islands(states, 0)
        r["chunk"] = c
        want.append(r)
    want = np.concatenate(want)
    print("island records:", len(want))
    assert len(want) > 20
    assert np.array_equal(recs, want)
    dpost = torch.from_numpy(post).to(dev)
    conf = D.contigs_island_confidence(gpu_ctx, dpost, b["span"], d["offs"], d["lens"], b["n"],
                                       out, cnt)
    torch.cuda.synchronize()
    gpu_ctx.sync()
    conf = conf.cpu().numpy()[: len(recs)]
    mean = np.array([post[int(b["offs"][r["chunk"]]) + int(r["beg1"]) - 1:][: int(r["len"])]
                     .astype(np.float64).mean() for r in recs])
    assert np.all(np.abs(conf - mean) <= 2.0 ** -23 * mean), (conf, mean)
    assert np.all((conf > 0.5) & (conf <= 1.0))


def test_confidence_range_errors(gpu_ctx, dev):
    import torch
    from cpgisland_amd import _lib
    from cpgisland_amd import device as D
    b, d = _batch(), _dev_batch(dev)
    post, _, _ = _outputs(gpu_ctx, dev, "initial")
    c = int(np.argmax(b["lens"]))                # the 66000-base contig
    L = int(b["lens"][c])
    recs = np.zeros(3, _lib.ISLAND_DTYPE)
    recs["beg1"] = [11, 1, L - 4]                # ok | contig index >= n | span past the end
    recs["len"] = [300, 200, 10]
    recs["chunk"] = [c, b["n"], c]
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(3, 32).copy()).to(dev)
    cnt = torch.tensor([3], dtype=torch.int64, device=dev)
    conf = D.contigs_island_confidence(gpu_ctx, torch.from_numpy(post).to(dev), b["span"],
                                       d["offs"], d["lens"], b["n"], d_recs, cnt)
    torch.cuda.synchronize()
    with pytest.raises(_lib.CpgInvalid):
        gpu_ctx.sync()
    gpu_ctx.sync()                               # the status word was cleared
    got = conf.cpu().numpy()
    o = int(b["offs"][c])
    want = post[o + 10: o + 310].astype(np.float64).mean()
    assert abs(got[0] - want) <= 2.0 ** -23 * want
    assert np.isnan(got[1]) and np.isnan(got[2])


def test_contract_errors(gpu_ctx, dev):
    import torch
    from cpgisland_amd import _lib
    b, d = _batch(), _dev_batch(dev)
    m = _model("initial")
    bad = m.copy()
    bad[72:76] = [0.9, 0.1, 0.0, 0.0]            # emission row of A+
    assert _run(gpu_ctx, dev, bad)[0] == _lib.CPG_E_UNSUPPORTED
    assert _run(gpu_ctx, dev, m, post_offset=1)[0] == _lib.CPG_E_INVALID      # d_post + 4 bytes
    gpu_ctx.sync()
    # contig 1 at an offset % 64 != 0, contig 2 longer than 2^20 (its bases need not exist: the
    # length fails before anything is read): both skipped, contigs 0 and 3 as in a batch of two
    offs = torch.tensor([0, 100, 256, 512], dtype=torch.int64, device=dev)
    lens = torch.tensor([90, 50, (1 << 20) + 1, 200], dtype=torch.int32, device=dev)
    rc, (post, sign, ll) = _run(gpu_ctx, dev, m, offs=offs, lens=lens, nbases=2 << 20)
    assert rc == _lib.CPG_OK
    with pytest.raises(_lib.CpgInvalid):
        gpu_ctx.sync()
    gpu_ctx.sync()                               # the status word was cleared
    rc, (p2, s2, l2) = _run(gpu_ctx, dev, m, offs=offs[[0, 3]].contiguous(),
                            lens=lens[[0, 3]].contiguous(), nbases=2 << 20)
    assert rc == _lib.CPG_OK
    gpu_ctx.sync()
    assert np.array_equal(post.view(np.int32), p2.view(np.int32)) and np.array_equal(sign, s2)
    assert np.array_equal(ll[[0, 3]].view(np.int64), l2.view(np.int64))
    assert np.isnan(ll[[1, 2]]).all() and np.isnan(post[128:512]).all()
    assert not np.isnan(post[:90]).any() and not np.isnan(post[512:712]).any()
