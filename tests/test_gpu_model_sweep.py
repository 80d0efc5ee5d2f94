"""The exact Viterbi scan swept over model families (oracle/families.py): every constant the
scan's exactness argument derives from the model (vit_prepare: qshift, eps, emin, emax,
tie_mask) takes values the reference's own model never gives it, at the smallest shapes that
take each launch path of launch_viterbi (k_viterbi.hip).  tests/test_model_families.py shows
on the CPU that each family reaches the path it is named for on these very chunks.

Every call goes through the C-ABI (device.viterbi, device.decode, device.islands,
HmmEvaluator.decode).  Compared against the C oracle chunk by chunk: state signs, best scores
as uint64 bit patterns (== cannot see a zero's sign), island records, a '-' tail, and a clean
ctx.sync() (no CPG_E_VERIFY).  One test id per (shape, family): the cases of a shape run back
to back on the session context with a different model each call (the per-model table caches
serve another model every time), and each shape ends by repeating its first case bitwise.

Which case a reverted rule breaks (tried on scratch builds of libcpg.so): with binade_ok
ignoring tie_mask, 16 ids fail, among them [64k_x3-tie15-synth], [64k_x3-tie12-synth],
[128k_x2-tie17-synth], [1m_x1-tie17-synth] and [64k_x3-random_norm1-synth] (random_norm1 and
3 have a tie binade of their own): the blocks inside the tie binade are planned REGULAR with a
constant rounded the wrong way.  With ref_step's '>' turned into '>=', 82 ids fail, among them
every symmetric and zero case past T = 1 (each step ties: the path flips from '+' to '-').
"""
import functools

import numpy as np
import pytest

from oracle import coracle as co
from oracle import families as fam

from test_gpu_parity import assert_estep_close
from test_model_families import SHAPES, sweep_bases

pytestmark = pytest.mark.gpu

CAP = 1 << 18
# an order in which neighbours are never two members of one family group
ALL = ["initial", "tie12", "near_one", "random_norm0", "symmetric", "tie15", "huge",
       "random_norm1", "all_one", "pi_tiny", "random_norm2", "zero", "tie17", "sym_blocks",
       "random_norm3", "pow2", "random_norm4", "pi_one", "random_norm5"]
assert sorted(ALL) == sorted(fam.names())
UNIFORM_TOO = ["symmetric", "all_one", "zero"]
SOME = ["tie17", "near_one", "symmetric", "huge", "zero", "random_norm0"]
FAMILIES_AT = {
    "64k_x3": ALL, "300b_x2": ALL,
    "128k_x2": SOME, "300b_part_x1": SOME, "1k_x9": SOME,
    "1m_x1": ["near_one", "tie17", "symmetric"],
    "64k_x257": ["symmetric", "tie15"],
}


def _cases():
    out = []
    for shape, names in FAMILIES_AT.items():
        cs = [(shape, n, "synth") for n in names]
        cs += [(shape, n, "uniform") for n in UNIFORM_TOO if n in names]
        out += [c + (False,) for c in cs] + [cs[0] + (True,)]
    return out


def _id(c):
    return "%s-%s-%s%s" % (c[0], c[1], c[2], "-again" if c[3] else "")


_DEV = {}          # (shape, src) -> packed bases on the device
_BITS = {}         # (shape, family, src) -> the first run's raw outputs


def _packed_dev(shape, src, dev):
    from cpgisland_amd import device as D
    if (shape, src) not in _DEV:
        packed = sweep_bases(shape, src)[0]
        _DEV[shape, src] = D.to_device(np.concatenate([packed, np.zeros(8, np.uint32)]), dev)
    return _DEV[shape, src]


def _sign_words(sign, nwords):
    """0/1 per position -> packed sign words (32 per uint32, LSB first), zero padded."""
    bits = np.zeros(nwords * 32, np.uint8)
    bits[:len(sign)] = sign
    return np.packbits(bits, bitorder="little").view("<u4")


@functools.lru_cache(maxsize=None)
def _reference(shape, name, src):
    """(sign words incl. the '-' tail, scores, island records) of the oracle's decode loop."""
    C, nch, tail = SHAPES[shape]
    obs = sweep_bases(shape, src)[1]
    m = fam.family(name)
    n = C * nch + tail
    if shape == "64k_x257":
        # viterbi2 per chunk, states as base + 4 * (1 - sign); viterbi8 on the first and last
        sign = np.zeros(nch * C, np.uint8)
        score = np.zeros(nch)
        recs = []
        for c in range(nch):
            o = obs[c * C:(c + 1) * C]
            sign[c * C:(c + 1) * C], score[c] = co.viterbi2(m, o)
            st = o.astype(np.int32) + 4 * (1 - sign[c * C:(c + 1) * C].astype(np.int32))
            if c in (0, nch - 1):
                st8, best8 = co.viterbi8(m, o)
                assert np.array_equal(st8, st)
                assert np.float64(best8).view(np.uint64) == score[c:c + 1].view(np.uint64)[0]
            recs.append(co.islands(st, c))
        isl = np.concatenate(recs)
    else:
        states, isl, score = co.decode_chunks(m, obs, C)
        sign = (states < 4).astype(np.uint8)
    return _sign_words(sign, (n + 31) // 32), score, isl


def _run_case(ctx, dev, shape, name, src):
    """One case on the GPU against the oracle; returns the raw outputs."""
    import torch
    from cpgisland_amd import HmmModel
    from cpgisland_amd import device as D
    C, nch, tail = SHAPES[shape]
    n = C * nch + tail
    w = (n + 31) // 32
    dp = _packed_dev(shape, src, dev)
    hm = HmmModel.from_struct(fam.family(name))
    ref_sign, ref_score, ref_isl = _reference(shape, name, src)
    what = (shape, name, src)

    so, sc = D.viterbi(ctx, hm, dp, n, C)
    torch.cuda.synchronize()
    ctx.sync()                                              # no CPG_E_VERIFY
    got_sign = so.cpu().numpy().view(np.uint32)[:w]
    got_score = sc.cpu().numpy()[:nch]
    assert np.array_equal(got_sign, ref_sign), what         # signs, and the tail all '-'
    assert np.array_equal(got_score.view(np.uint64), ref_score.view(np.uint64)), what
    out = [got_sign, got_score.view(np.uint64)]
    if C % 32:                   # islands take chunk lengths that are multiples of 32
        return out

    so2, sc2, io, ic = D.decode(ctx, hm, dp, n, C, cap=CAP)
    torch.cuda.synchronize()
    ctx.sync()
    assert int(ic.item()) <= CAP
    got_isl = D.islands_to_numpy(io, ic)
    assert np.array_equal(so2.cpu().numpy().view(np.uint32)[:w], ref_sign), what
    assert np.array_equal(sc2.cpu().numpy()[:nch].view(np.uint64),
                          ref_score.view(np.uint64)), what
    assert np.array_equal(got_isl, ref_isl), what
    out.append(got_isl.view(np.uint8))

    if shape in ("64k_x3", "300b_x2"):
        # the fused call bitwise the two single calls, chunk numbering from 7
        so7, sc7, io7, ic7 = D.decode(ctx, hm, dp, n, C, cap=CAP, first_chunk=7)
        io3, ic3 = D.islands(ctx, dp, so, n, C, cap=CAP, first_chunk=7)
        torch.cuda.synchronize()
        ctx.sync()
        assert np.array_equal(so7.cpu().numpy().view(np.uint32)[:w], got_sign), what
        assert np.array_equal(sc7.cpu().numpy()[:nch].view(np.uint64),
                              got_score.view(np.uint64)), what
        isl7 = D.islands_to_numpy(io7, ic7)
        assert np.array_equal(isl7, D.islands_to_numpy(io3, ic3)), what
        assert np.array_equal(isl7["chunk"], got_isl["chunk"] + 7), what
    return out


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_sweep_decode(gpu_ctx, torch_dev, case):
    shape, name, src, again = case
    got = _run_case(gpu_ctx, torch_dev, shape, name, src)
    if not again:
        _BITS[shape, name, src] = got
        return
    # the shape's first case once more, after every other model went through the table caches
    first = _BITS.get((shape, name, src)) or _run_case(gpu_ctx, torch_dev, shape, name, src)
    assert len(first) == len(got)
    for a, b in zip(first, got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("T", [1, 2, 257, 4097, 100003])
@pytest.mark.parametrize("name", ALL)
def test_sweep_evaluator_decode(gpu_ctx, name, T):
    from cpgisland_amd import HmmEvaluator, HmmModel
    m = fam.family(name)
    obs = sweep_bases("64k_x3")[1][:T]
    st = HmmEvaluator.decode(HmmModel.from_struct(m), obs.astype(np.int32), True, ctx=gpu_ctx)
    gpu_ctx.sync()
    ref, _ = co.viterbi8(m, obs)
    assert st.dtype == ref.dtype and np.array_equal(st, ref)


# ---------------------------------------------------------------- E-step
ESTEP_FAMILIES = ["random_norm0", "pow2", "random_norm1", "symmetric", "random_norm2", "pi_one"]


@functools.lru_cache(maxsize=None)
def _estep_bases():
    from cpgisland_amd import device as D
    from oracle import pyref as pr
    n = 4 * 65536
    packed, _ = D.synth_host(7100, 0, n)
    return packed, pr.unpack(packed, n)


@pytest.mark.parametrize("C", [4096, 65536])
@pytest.mark.parametrize("name", ESTEP_FAMILIES)
def test_sweep_estep(gpu_ctx, torch_dev, name, C):
    """bw_estep on the families with normalised rows (the model-dependent part: the kernel's
    rescaling exponents), four chunks, against the oracle under the suite's own criterion."""
    import torch
    from cpgisland_amd import HmmModel
    from cpgisland_amd import device as D
    m = fam.normalised_rows(fam.family(name))
    a = m[8:72].reshape(8, 8)
    assert np.allclose(a.sum(axis=1), 1.0, rtol=1e-15, atol=0) and a.min() >= 1e-9
    n = 4 * C
    packed, obs = _estep_bases()
    obs = obs[:n]
    if ("estep", C) not in _DEV:
        _DEV["estep", C] = D.to_device(
            np.concatenate([packed[:n // 16], np.zeros(8, np.uint32)]), torch_dev)
    dp = _DEV["estep", C]
    hm = HmmModel.from_struct(m)
    e1 = D.bw_estep(gpu_ctx, hm, dp, n, C).cpu().numpy()
    e2 = D.bw_estep(gpu_ctx, hm, dp, n, C).cpu().numpy()
    torch.cuda.synchronize()
    gpu_ctx.sync()
    assert np.array_equal(e1.view(np.uint64), e2.view(np.uint64))
    assert_estep_close(e1, co.estep(m, obs, C), obs, C, (name, C))
