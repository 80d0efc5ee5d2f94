"""The model families of oracle/families.py (CPU only): each family reaches the path of the
exact Viterbi scan it is named for, on the very chunks tests/test_gpu_model_sweep.py decodes,
and the oracle those GPU tests compare against holds on them (C restatement == Python
restatement == brute force), the tie families above all: the restatements' first-index
tie-break has otherwise only met ties by accident.
"""
import functools

import numpy as np
import pytest

from oracle import coracle as co
from oracle import families as fam
from oracle import pyref as pr

from test_oracle import brute_force_check

K_MAX_STAGED_BAR = 64      # kMaxStagedBar, k_viterbi.hip: barriers K4 stages in LDS per chunk

# name -> (chunk length, whole chunks, tail bases): the smallest inputs that take each launch
# path of launch_viterbi (k_viterbi.hip), see tests/test_gpu_model_sweep.py
SHAPES = {
    "64k_x3": (65536, 3, 777),      # segment path, one segment; K6 fused in K5; fused islands
    "128k_x2": (131072, 2, 0),      # two segments: segment products, k_vit_segplan's look-back
    "300b_x2": (76800, 2, 0),       # 300 blocks: k_vit_scan / k_vit_chain, k_vit_tscan
    "300b_part_x1": (76700, 1, 0),  # a partly filled last block
    "1k_x9": (1024, 9, 0),          # chunks of a few blocks
    "1m_x1": (1 << 20, 1, 0),       # the reference's 16-segment chunk
    "64k_x257": (65536, 257, 0),    # past tail_fusion_pays
}


@functools.lru_cache(maxsize=None)
def sweep_bases(shape, src="synth"):
    """(packed uint32[], bases uint8[N]) of a sweep shape: the synthetic genome (cpg_synth) or
    uniform random bases, seeded by the shape."""
    from cpgisland_amd import device as D
    C, nch, tail = SHAPES[shape]
    n = C * nch + tail
    seed = 7000 + sorted(SHAPES).index(shape)
    if src == "synth":
        packed, _ = D.synth_host(seed, 0, n)
        obs = pr.unpack(packed, n)
    else:
        obs = np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)
        packed = np.concatenate([pr.pack(obs), np.zeros(4, np.uint32)])
    obs.setflags(write=False)
    packed.setflags(write=False)
    return packed, obs


@functools.lru_cache(maxsize=None)
def chunk_profile(name, shape="64k_x3", src="synth"):
    """profile() of the family on the first chunk of a sweep shape."""
    C = SHAPES[shape][0]
    return fam.profile(fam.family(name), sweep_bases(shape, src)[1][:C])


# ---------------------------------------------------------------- the families' contract
@pytest.mark.parametrize("name", fam.names())
def test_family_is_inside_the_fast_path_contract(name):
    """vit_fast_ok (cpg_host.cpp): deterministic emissions, 0 <= pi <= 1, 0 < a <= 1."""
    pi, a, b = co.model_split(fam.family(name))
    assert np.array_equal(b, pr.INITIAL_B)
    assert np.all((pi >= 0) & (pi <= 1)) and np.all((a > 0) & (a <= 1))
    assert np.array_equal(fam.family(name), fam.family(name))      # seeded


def test_prepare_restates_the_initial_model_constants():
    """The documented constants of the reference's model at the training chunk length."""
    p = fam.prepare(fam.family("initial"), 65536)
    assert p["qshift"] == 18 and p["emin"] == 8 and not (p["ties"] & set(range(8, 21)))


# ---------------------------------------------------------------- witnesses
@pytest.mark.parametrize("name", ["tie15", "huge"])
def test_witness_more_irregular_blocks_than_k4_stages(name):
    assert chunk_profile(name)["irregular"] > K_MAX_STAGED_BAR


@pytest.mark.parametrize("name", ["near_one", "all_one"])
def test_witness_every_block_irregular(name):
    p = chunk_profile(name)
    assert p["nblocks"] == 256 and p["irregular"] == p["nblocks"] - 1


@pytest.mark.parametrize("e", fam.TIE_BINADES)
def test_witness_tie_binade_is_crossed(e):
    a = fam.tie_constant(e)
    u = 2.0 ** (e - 52)
    r = np.log(a) / u
    assert r - np.floor(r) == 0.5
    p = chunk_profile("tie%d" % e, "128k_x2" if e == 17 else "64k_x3")
    assert e in p["tie_binades"] and e >= p["emin"]
    assert e - 1 in p["binades"] and e in p["binades"]       # delta crosses into it


@pytest.mark.parametrize("name,src", [("symmetric", "synth"), ("symmetric", "uniform"),
                                      ("sym_blocks", "synth")])
def test_witness_tie_at_every_step_and_at_the_end(name, src):
    p = chunk_profile(name, "64k_x3", src)
    assert p["ties"] == 65535 and p["final_tie"]


@pytest.mark.parametrize("name", ["all_one", "zero"])
def test_witness_all_one_ties_every_step(name):
    p = chunk_profile(name, "64k_x3", "uniform")
    # all_one: log pi+ != log pi-, so the first step has no tie; every later one has
    assert p["ties"] == (65535 if name == "zero" else 65534)
    if name == "zero":
        assert p["final_tie"] and p["score"] == 0.0 and not np.signbit(p["score"])


def test_witness_pow2_ties():
    assert chunk_profile("pow2")["ties"] >= 1000


def test_witness_qshift_extremes():
    assert chunk_profile("huge")["qshift"] <= 12
    assert chunk_profile("near_one")["qshift"] == 24
    assert chunk_profile("near_one")["emin"] == chunk_profile("near_one")["emax"] == 4


def test_witness_pi_tiny_starts_in_binade_9():
    m = fam.family("pi_tiny")
    assert {int(np.floor(np.log2(-x))) for x in np.log(m[:8])} == {9, 8}    # 690.8, 460.5


# ---------------------------------------------------------------- the oracle on the families
def _obs(T, seed):
    return np.random.default_rng(seed).integers(0, 4, T).astype(np.uint8)


@pytest.mark.parametrize("T", [1, 2, 257, 2000])
@pytest.mark.parametrize("name", fam.names())
def test_oracle_c_vs_python_on_family(name, T):
    m = fam.family(name)
    pi, a, b = co.model_split(m)
    for obs in (_obs(T, T), sweep_bases("1k_x9")[1][:T] if T <= 1024 else sweep_bases("64k_x3")[1][:T]):
        st, best = co.viterbi8(m, obs)
        seq, mp = pr.viterbi8(pi.tolist(), a.tolist(), b.tolist(), obs.tolist())
        assert list(st) == seq
        assert pr.f64_bits(best) == pr.f64_bits(mp)
        sg, b2 = co.viterbi2(m, obs)
        assert np.array_equal(sg, (st < 4).astype(np.uint8))
        assert pr.f64_bits(b2) == pr.f64_bits(best)


@pytest.mark.parametrize("name", fam.names())
def test_oracle_brute_force_on_family(name):
    m = fam.family(name)
    for T in (2, 5, 10):
        brute_force_check(m, _obs(T, 10 * T))
