// k_posterior.hip — posterior decoding on gfx950: for every position p of every whole chunk,
// P(state_p in {A+,C+,G+,T+} | the whole chunk, model), the maximum-posterior path as sign
// bits, the chunk log-likelihood; and the mean posterior of island records ("confidence").
//
// The chain is the E-step's (k_estep.hip): with the deterministic emission matrix two states
// are live per position, so forward and backward are products of 2x2 positive matrices M_p
// (rows: previous state +/-, cols: current state), rescaled by exact powers of two.  A chunk
// may be longer than one workgroup's 65,536 positions (the decode chunk is 1 Mi), so it is cut
// into SEGMENTS of at most 65,536 positions (1024 lanes x 64 positions):
//   A. k_post_seg:  every segment's matrix product (lane products, workgroup reduction);
//   B. k_post_scan: one lane per chunk walks its segment products with vectors — alpha entering
//      and beta leaving every segment, and the chunk log-likelihood;
//   C. k_post_emit: per segment, the lane products again (the bases cost 0.25 B per base to
//      re-read; cheaper than storing 64 KiB of products per segment), wave scans seeded with
//      B's vectors, then every lane walks its 64 positions in 16-position mini-blocks, last to
//      first: alphas recomputed into registers from a checkpoint, then the backward chain with
//      p+ = alpha+ beta+ / (alpha+ beta+ + alpha- beta-)  (any per-position scale cancels).
// A lane's 64 posteriors are 256 contiguous bytes, a wave's store from the walk would be
// lane-strided: two mini-blocks (32 floats per lane) are staged in the wave's LDS tile and
// written out as 16 B per lane, eight whole 128-B lines per store instruction.
// No kernel waits for another workgroup; no reduction depends on an order: results are
// bitwise reproducible.  The helpers (Mat, DPP moves, vnorm) are k_estep.hip's, copied: the
// E-step's own code stays as it is.

#include <cmath>

#include "cpg_internal.h"

// a tolerance-bound fp64 computation, like the E-step: products and sums may contract to FMAs
#pragma clang fp contract(fast)

namespace cpg {
namespace {

constexpr int kPT = 1024;                            // max lanes per segment
constexpr int kLanePos = 64;                         // positions per lane
constexpr int64_t kSeg = (int64_t)kPT * kLanePos;    // positions per segment
constexpr int kMB = 16;                              // positions per mini-block (one packed word)
constexpr int kIdent = 16;                           // table row of the identity matrix
// the wave's staging tile: 64 lanes x 32 floats, rows padded to 36 floats (144 B: 16-B aligned,
// a column of 8 lanes' 16-B stores falls on 8 different bank quads)
constexpr int kStageRow = 36;
constexpr int kStageWave = 64 * kStageRow;           // floats per wave

struct Mat {
    double a, b, c, d;   // [[a b] [c d]]
    int e;               // value = 2^e * matrix
};

// floor(log2 mx) for finite mx > 0 (denormals included), 0 for mx == 0 — a select, not a branch
__device__ __forceinline__ int exp2_floor(double mx) {
    const int k = __builtin_amdgcn_frexp_exp(mx) - 1;
    return mx > 0.0 ? k : 0;
}
__device__ __forceinline__ void mnorm(Mat& m) {
    const double mx = fmax(fmax(m.a, m.b), fmax(m.c, m.d));
    const int k = exp2_floor(mx);
    m.a = ldexp(m.a, -k); m.b = ldexp(m.b, -k); m.c = ldexp(m.c, -k); m.d = ldexp(m.d, -k);
    m.e += k;
}
__device__ __forceinline__ Mat mmul(const Mat& x, const Mat& y) {
    Mat r{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c,
          x.c * y.b + x.d * y.d, x.e + y.e};
    mnorm(r);
    return r;
}
// product without the renormalisation (inside a scan of normalised products two or three
// unnormalised levels stay far inside fp64's range)
__device__ __forceinline__ Mat mmul_nn(const Mat& x, const Mat& y) {
    return {x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c,
            x.c * y.b + x.d * y.d, x.e + y.e};
}
__device__ __forceinline__ Mat mid() { return {1.0, 0.0, 0.0, 1.0, 0}; }
// DPP moves: CTRL 0x110+n = row_shr:n, 0x100+n = row_shl:n (inside 16-lane rows); lanes
// without a source take `old`
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v, double old) {
    const long long vi = __double_as_longlong(v), oi = __double_as_longlong(old);
    const int lo = __builtin_amdgcn_update_dpp((int)oi, (int)vi, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(oi >> 32), (int)(vi >> 32), CTRL, 0xF, 0xF,
                                               false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int CTRL>
__device__ __forceinline__ Mat dpp_mat(const Mat& x, const Mat& old) {
    return {dpp_f64<CTRL>(x.a, old.a), dpp_f64<CTRL>(x.b, old.b), dpp_f64<CTRL>(x.c, old.c),
            dpp_f64<CTRL>(x.d, old.d),
            __builtin_amdgcn_update_dpp(old.e, x.e, CTRL, 0xF, 0xF, false)};
}
// x from the lane `off` below (up) / above (down) inside its 16-lane row, identity where there
// is none
__device__ __forceinline__ Mat row_up(const Mat& x, int off) {
    const Mat I = {1.0, 0.0, 0.0, 1.0, 0};
    switch (off) {
        case 1: return dpp_mat<0x111>(x, I);
        case 2: return dpp_mat<0x112>(x, I);
        case 4: return dpp_mat<0x114>(x, I);
        default: return dpp_mat<0x118>(x, I);
    }
}
__device__ __forceinline__ Mat row_down(const Mat& x, int off) {
    const Mat I = {1.0, 0.0, 0.0, 1.0, 0};
    switch (off) {
        case 1: return dpp_mat<0x101>(x, I);
        case 2: return dpp_mat<0x102>(x, I);
        case 4: return dpp_mat<0x104>(x, I);
        default: return dpp_mat<0x108>(x, I);
    }
}
__device__ __forceinline__ Mat msel(bool c, const Mat& x, const Mat& y) {   // field selects
    return {c ? x.a : y.a, c ? x.b : y.b, c ? x.c : y.c, c ? x.d : y.d, c ? x.e : y.e};
}
__device__ __forceinline__ Mat shfl_mat(const Mat& x, int src) {
    return {__shfl(x.a, src), __shfl(x.b, src), __shfl(x.c, src), __shfl(x.d, src),
            __shfl(x.e, src)};
}
__device__ __forceinline__ Mat shfl_up_mat(const Mat& x, int d) {
    return {__shfl_up(x.a, d), __shfl_up(x.b, d), __shfl_up(x.c, d), __shfl_up(x.d, d),
            __shfl_up(x.e, d)};
}
__device__ __forceinline__ Mat shfl_down_mat(const Mat& x, int d) {
    return {__shfl_down(x.a, d), __shfl_down(x.b, d), __shfl_down(x.c, d), __shfl_down(x.d, d),
            __shfl_down(x.e, d)};
}
__device__ __forceinline__ int vnorm(double& x, double& y) {   // returns the shift applied
    const int k = exp2_floor(fmax(x, y));
    x = ldexp(x, -k);
    y = ldexp(y, -k);
    return k;
}

// inclusive prefix (xp) and suffix (xs) products of the wave's 64 lane products: DPP inside
// 16-lane rows, then the row totals across the rows
template <bool kSuffix>
__device__ __forceinline__ void wave_scan(const Mat& P, int lane, Mat& xp, Mat& xs) {
    xp = P;
    xs = P;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const Mat yp = row_up(xp, off);
        xp = off < 8 ? mmul_nn(yp, xp) : mmul(yp, xp);
        if (kSuffix) {
            const Mat ys = row_down(xs, off);
            xs = off < 8 ? mmul_nn(xs, ys) : mmul(xs, ys);
        }
    }
    // across the rows: a lane's in-row prefix times the TOTALS of the rows before it (lanes 15,
    // 31, 47 hold them), its in-row suffix times the totals of the rows after it (lanes 16, 32,
    // 48).  (Not a shift by 16 / 32 lanes: lane r - 16 holds only its row's prefix up to its
    // own column, so the product would skip the rest of that row — an error that the chain
    // forgets within a few hundred positions, invisible in sums, visible per position.)
    const int row = lane >> 4;
    {
        const Mat t0 = shfl_mat(xp, 15), t1 = shfl_mat(xp, 31), t2 = shfl_mat(xp, 47);
        const Mat t01 = mmul(t0, t1), t012 = mmul(t01, t2);
        const Mat pre = msel(row == 1, t0, msel(row == 2, t01, t012));
        const Mat y = mmul(pre, xp);
        xp = msel(row == 0, xp, y);
    }
    if (kSuffix) {
        const Mat s1 = shfl_mat(xs, 16), s2 = shfl_mat(xs, 32), s3 = shfl_mat(xs, 48);
        const Mat s23 = mmul(s2, s3), s123 = mmul(s1, s23);
        const Mat post = msel(row == 2, s3, msel(row == 1, s23, s123));
        const Mat y = mmul(xs, post);
        xs = msel(row == 3, xs, y);
    }
}

// where a workgroup stands: chunk c, segment sg of nseg, C positions per chunk
struct Geo {
    int64_t c, seg0;      // chunk, the segment's first position in the chunk
    int64_t wpc;          // packed words per chunk
};

// the lane's 64 bases (4 packed words) and the word before them; words past the chunk's last
// read as 0 (their positions are past the end: identity, no output)
struct Bases {
    uint32_t r0, r1, r2, r3, prev;   // (scalars: selected by mini-block, never indexed)
};
__device__ __forceinline__ Bases lane_bases(const uint32_t* __restrict__ pk, int64_t w0,
                                            int64_t wpc) {
    Bases b;
    if (w0 + 4 <= wpc) {
        const uint4 v = *reinterpret_cast<const uint4*>(pk + w0);
        b.r0 = v.x; b.r1 = v.y; b.r2 = v.z; b.r3 = v.w;
    } else {
        b.r0 = w0 < wpc ? pk[w0] : 0u;
        b.r1 = w0 + 1 < wpc ? pk[w0 + 1] : 0u;
        b.r2 = w0 + 2 < wpc ? pk[w0 + 2] : 0u;
        b.r3 = w0 + 3 < wpc ? pk[w0 + 3] : 0u;
    }
    b.prev = (w0 > 0 && w0 <= wpc) ? pk[w0 - 1] : 0u;
    return b;
}
// the 16 table rows of mini-block m as 4-bit fields are taken from cm: base i-1 at bits 2i,
// base i at bits 2i+2, so row_i = (cm >> 2i) & 15 = prev | cur << 2
__device__ __forceinline__ uint64_t mb_codes(uint32_t xw, uint32_t pw) {
    return ((uint64_t)xw << 2) | (pw >> 30);
}

// the model's one-step rows (est_tables: TA[d] = (M(+,+), M(+,-)), TB[d] = (M(-,+), M(-,-)),
// d = previous base | current base << 2) and the identity as row 16, into LDS
__device__ __forceinline__ void load_rows(double2* TA, double2* TB,
                                          const double2* __restrict__ gtab) {
    const int t = threadIdx.x;
    if (t < 16) {
        TA[t] = gtab[t];
        TB[t] = gtab[16 + t];
    }
    if (t == 16) {
        TA[kIdent] = make_double2(1.0, 0.0);
        TB[kIdent] = make_double2(0.0, 1.0);
    }
}

// the product of the lane's matrices: position j of the lane carries M_row, the identity when
// it is past the chunk's end (j >= nvl) or the chunk's first position (no transition into it).
// Four positions are multiplied raw, then into the running (normalised) product.  The
// mini-block loop is kept rolled (registers: unrolled, the compiler hoists 64 positions' rows).
__device__ __forceinline__ uint32_t word_of(const Bases& bs, int m) {   // raw[m]; raw[-1] = prev
    return m < 0 ? bs.prev : m == 0 ? bs.r0 : m == 1 ? bs.r1 : m == 2 ? bs.r2 : bs.r3;
}
__device__ __forceinline__ Mat lane_product(const Bases& bs, int nvl, bool first,
                                            const double2* TA, const double2* TB) {
    Mat P = mid();
#pragma unroll 1
    for (int m = 0; m < kLanePos / kMB; ++m) {
        const uint64_t cm = mb_codes(word_of(bs, m), word_of(bs, m - 1));
        const int nv = nvl - kMB * m;
        const bool f0 = first && m == 0;
#pragma unroll
        for (int g = 0; g < kMB / 4; ++g) {
            double x00 = 1.0, x01 = 0.0, x10 = 0.0, x11 = 1.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = 4 * g + k;
                uint32_t d = (uint32_t)(cm >> (2 * i)) & 15u;
                if (i >= nv || (i == 0 && f0)) d = kIdent;
                const double2 ma = TA[d], mb = TB[d];
                if (k == 0) {
                    x00 = ma.x; x01 = ma.y; x10 = mb.x; x11 = mb.y;
                } else {
                    const double n00 = x00 * ma.x + x01 * mb.x, n01 = x00 * ma.y + x01 * mb.y;
                    const double n10 = x10 * ma.x + x11 * mb.x, n11 = x10 * ma.y + x11 * mb.y;
                    x00 = n00; x01 = n01; x10 = n10; x11 = n11;
                }
            }
            P = mmul(P, Mat{x00, x01, x10, x11, 0});
        }
    }
    return P;
}

__device__ __forceinline__ Geo geo_of(int64_t C, int nseg) {
    Geo g;
    g.c = blockIdx.x / (unsigned)nseg;
    g.seg0 = (int64_t)(blockIdx.x % (unsigned)nseg) * kSeg;
    g.wpc = (C + 15) / 16;
    return g;
}

// A. the segment's matrix product -> segP[chunk * nseg + segment]
__global__ __launch_bounds__(kPT) void k_post_seg(const double2* __restrict__ gtab,
                                                  const uint32_t* __restrict__ packed, int64_t C,
                                                  int nseg, Mat* __restrict__ segP) {
    __shared__ __attribute__((aligned(16))) double2 TA[32], TB[32];
    __shared__ Mat sTot[kPT / 64];
    const Geo g = geo_of(C, nseg);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = blockDim.x >> 6;
    load_rows(TA, TB, gtab);
    const int64_t p0 = g.seg0 + (int64_t)t * kLanePos;   // the lane's first position in the chunk
    const Bases bs = lane_bases(packed + g.c * g.wpc, p0 / 16, g.wpc);
    const int nvl = (int)(C - p0 > kLanePos ? kLanePos : (C - p0 < 0 ? 0 : C - p0));
    __syncthreads();
    const Mat P = lane_product(bs, nvl, p0 == 0, TA, TB);
    Mat xp, xs;
    wave_scan<false>(P, lane, xp, xs);
    if (lane == 63) sTot[wave] = xp;
    __syncthreads();
    if (t == 0) {
        Mat T = sTot[0];
        for (int w = 1; w < nw; ++w) T = mmul(T, sTot[w]);
        segP[blockIdx.x] = T;
    }
}

// B. one lane per chunk: alpha entering and beta leaving every segment, the log-likelihood
__global__ __launch_bounds__(256) void k_post_scan(const cpg_model model,
                                                   const uint32_t* __restrict__ packed,
                                                   int64_t nch, int64_t C, int nseg,
                                                   const Mat* __restrict__ segP,
                                                   double2* __restrict__ ain,
                                                   double2* __restrict__ bout,
                                                   double* __restrict__ loglik) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nch) return;
    const uint32_t o0 = packed[c * ((C + 15) / 16)] & 3u;
    double vP = model.pi[o0], vM = model.pi[o0 + 4];   // alpha_0 (b = 1 when live)
    const Mat* sp = segP + c * nseg;
    long long e = 0;
    for (int s = 0; s < nseg; ++s) {
        e += vnorm(vP, vM);
        ain[c * nseg + s] = make_double2(vP, vM);
        const Mat m = sp[s];
        const double nP = vP * m.a + vM * m.c, nM = vP * m.b + vM * m.d;
        vP = nP;
        vM = nM;
        e += m.e;
    }
    e += vnorm(vP, vM);
    // P(chunk | model) = 0 (both live states of the first base at pi = 0): log 0 = -inf
    if (loglik) loglik[c] = log(vP + vM) + (double)e * 0.69314718055994530942;
    double uP = 1.0, uM = 1.0;
    for (int s = nseg - 1; s >= 0; --s) {
        bout[c * nseg + s] = make_double2(uP, uM);
        const Mat m = sp[s];
        const double nP = m.a * uP + m.b * uM, nM = m.c * uP + m.d * uM;
        uP = nP;
        uM = nM;
        vnorm(uP, uM);
    }
}

// C. per segment: the posteriors and the maximum-posterior path
template <bool kPost, bool kSign>
__global__ __launch_bounds__(kPT) void k_post_emit(const double2* __restrict__ gtab,
                                                   const uint32_t* __restrict__ packed, int64_t C,
                                                   int nseg, const double2* __restrict__ ain,
                                                   const double2* __restrict__ bout,
                                                   float* __restrict__ post,
                                                   uint32_t* __restrict__ sign) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2* TA = reinterpret_cast<double2*>(smem);       // 17 rows used of 32
    double2* TB = TA + 32;
    Mat* sTot = reinterpret_cast<Mat*>(TB + 32);          // [16] wave totals
    float* stage = reinterpret_cast<float*>(smem + 2048); // [waves][64][kStageRow]
    const Geo g = geo_of(C, nseg);
    const int t = threadIdx.x, lane = t & 63, nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    load_rows(TA, TB, gtab);
    const int64_t p0 = g.seg0 + (int64_t)t * kLanePos;
    const Bases bs = lane_bases(packed + g.c * g.wpc, p0 / 16, g.wpc);
    const int nvl = (int)(C - p0 > kLanePos ? kLanePos : (C - p0 < 0 ? 0 : C - p0));
    const bool first = p0 == 0;
    __syncthreads();
    // 1. the lane product; 2. alpha entering / beta leaving the lane
    const Mat P = lane_product(bs, nvl, first, TA, TB);
    double aP, aM, bP, bM;
    {
        Mat xp, xs;
        wave_scan<true>(P, lane, xp, xs);
        if (lane == 63) sTot[wave] = xp;
        Mat ep = shfl_up_mat(xp, 1), es = shfl_down_mat(xs, 1);   // lanes before / after
        if (lane == 0) ep = mid();
        if (lane == 63) es = mid();
        __syncthreads();
        const double2 a0 = ain[blockIdx.x], b0 = bout[blockIdx.x];
        double vP = a0.x, vM = a0.y;       // alpha entering the wave: the waves before
        for (int w = 0; w < wave; ++w) {
            const Mat m = sTot[w];
            const double nP = vP * m.a + vM * m.c, nM = vP * m.b + vM * m.d;
            vP = nP;
            vM = nM;
            vnorm(vP, vM);
        }
        double uP = b0.x, uM = b0.y;       // beta leaving the wave: the waves after
        for (int w = nw - 1; w > wave; --w) {
            const Mat m = sTot[w];
            const double nP = m.a * uP + m.b * uM, nM = m.c * uP + m.d * uM;
            uP = nP;
            uM = nM;
            vnorm(uP, uM);
        }
        aP = vP * ep.a + vM * ep.c;
        aM = vP * ep.b + vM * ep.d;
        vnorm(aP, aM);
        bP = es.a * uP + es.b * uM;
        bM = es.c * uP + es.d * uM;
        vnorm(bP, bM);
    }
    // the alpha checkpoints: alpha entering mini-blocks 1..3, one forward walk with vectors
    // (mini-block 0's is alpha entering the lane)
    double c1P = 0.0, c1M = 0.0, c2P = 0.0, c2M = 0.0, c3P = 0.0, c3M = 0.0;
    {
        double xP = aP, xM = aM;
#pragma unroll 1
        for (int m = 0; m < kLanePos / kMB - 1; ++m) {
            const uint64_t cm = mb_codes(word_of(bs, m), word_of(bs, m - 1));
            const int nv = nvl - kMB * m;
            const bool f0 = first && m == 0;
#pragma unroll
            for (int i = 0; i < kMB; ++i) {
                uint32_t d = (uint32_t)(cm >> (2 * i)) & 15u;
                if (i >= nv || (i == 0 && f0)) d = kIdent;
                const double2 ma = TA[d], mb = TB[d];
                const double nP = xP * ma.x + xM * mb.x, nM = xP * ma.y + xM * mb.y;
                xP = nP;
                xM = nM;
                if (i % 4 == 3) vnorm(xP, xM);
            }
            if (m == 0) { c1P = xP; c1M = xM; }
            if (m == 1) { c2P = xP; c2M = xM; }
            if (m == 2) { c3P = xP; c3M = xM; }
        }
    }
    // 3. mini-blocks, last to first
    double yP = bP, yM = bM;   // beta at the mini-block's last position
    float* tile = stage + wave * kStageWave;
    uint32_t sbits = 0u, sw1 = 0u;
    const int64_t cbase = g.c * C;   // the chunk's first position in the output
#pragma unroll 1
    for (int m = kLanePos / kMB - 1; m >= 0; --m) {
        // (selects, not indexed registers)
        double xP = m == 0 ? aP : m == 1 ? c1P : m == 2 ? c2P : c3P;
        double xM = m == 0 ? aM : m == 1 ? c1M : m == 2 ? c2M : c3M;
        const uint64_t cm = mb_codes(word_of(bs, m), word_of(bs, m - 1));
        const int nv = nvl - kMB * m;             // valid positions of the mini-block (may be <= 0)
        const bool f0 = first && m == 0;
        auto rowi = [&](int i) -> uint32_t {   // i compile-time
            const uint32_t d = (uint32_t)(cm >> (2 * i)) & 15u;
            return (i >= nv || (i == 0 && f0)) ? (uint32_t)kIdent : d;
        };
        double alP[kMB], alM[kMB];
#pragma unroll
        for (int i = 0; i < kMB; ++i) {
            const uint32_t d = rowi(i);
            const double2 ma = TA[d], mb = TB[d];
            const double nP = xP * ma.x + xM * mb.x, nM = xP * ma.y + xM * mb.y;
            xP = nP;
            xM = nM;
            if (i % 4 == 3) vnorm(xP, xM);
            alP[i] = xP;
            alM[i] = xM;
            if (i % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
        const int half = m & 1;
        float4* row = reinterpret_cast<float4*>(tile + lane * kStageRow + 16 * half);
        float pv[4];
        uint32_t bits = 0u;
#pragma unroll
        for (int i = kMB - 1; i >= 0; --i) {
            const double qP = alP[i] * yP, qM = alM[i] * yM, den = qP + qM;
            if (kPost) pv[i % 4] = den > 0.0 ? (float)(qP / den) : 0.0f;
            if (kSign) bits |= (i < nv && qP > qM) ? (1u << i) : 0u;
            const uint32_t d = rowi(i);
            const double2 ma = TA[d], mb = TB[d];
            const double nP = ma.x * yP + ma.y * yM, nM = mb.x * yP + mb.y * yM;
            yP = nP;
            yM = nM;
            if (i % 4 == 0) {
                vnorm(yP, yM);
                if (kPost) row[i / 4] = make_float4(pv[0], pv[1], pv[2], pv[3]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        sbits |= bits << (16 * half);
        if (half == 0) {   // both mini-blocks of positions [32 h, 32 h + 32) of every lane
            const int h = m >> 1;
            if (kPost) {
                __syncthreads();
                // instruction k: lanes-rows 8k .. 8k+7 of the tile, 128 B each
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int idx = k * 64 + lane, l = idx >> 3, q = idx & 7;
                    const float4 v = *reinterpret_cast<const float4*>(tile + l * kStageRow + 4 * q);
                    const int64_t pos = g.seg0 + ((int64_t)(wave * 64 + l)) * kLanePos + 32 * h + 4 * q;
                    float* o = post + cbase + pos;
                    if (pos + 3 < C) {
                        *reinterpret_cast<float4*>(o) = v;
                    } else {
                        if (pos < C) o[0] = v.x;
                        if (pos + 1 < C) o[1] = v.y;
                        if (pos + 2 < C) o[2] = v.z;
                    }
                }
                __syncthreads();
            }
            if (h == 1) sw1 = sbits;
            sbits = h == 1 ? 0u : sbits;
        }
    }
    if (kSign) {   // the lane's two sign words (sbits: positions 0..31, sw1: 32..63)
        const int64_t nwords = (C + 31) / 32, wi = p0 / 32;
        uint32_t* o = sign + g.c * nwords + wi;
        if (wi + 1 < nwords) {
            *reinterpret_cast<uint2*>(o) = make_uint2(sbits, sw1);
        } else if (wi < nwords) {
            o[0] = sbits;
        }
    }
}

// Island confidence: one wave per record, the mean of post over the record's span.  The span
// from the record itself: chunk-local start = (uint32)(beg1 - 1) - (uint32)chunk * (uint32)C
// (the int32-wrapped coordinates of the reference unwrap modulo 2^32), length = len, buffer
// chunk = chunk - first_chunk.  A record outside the buffer: NaN and the status bit.
__global__ __launch_bounds__(256) void k_island_conf(const float* __restrict__ post,
                                                     int64_t nch, int64_t C, int64_t first_chunk,
                                                     const cpg_island* __restrict__ isl,
                                                     const int64_t* __restrict__ d_count,
                                                     int64_t cap, float* __restrict__ conf,
                                                     uint32_t* __restrict__ status) {
    int64_t n = *d_count;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nwaves) {
        const cpg_island r = isl[i];
        const uint32_t start = ((uint32_t)r.beg1 - 1u) - (uint32_t)r.chunk * (uint32_t)C;
        const int64_t bc = (int64_t)r.chunk - first_chunk;
        const bool ok = bc >= 0 && bc < nch && r.len >= 1 && (int64_t)start + r.len <= C;
        if (!ok) {
            if (lane == 0) {
                conf[i] = __builtin_nanf("");
                atomicOr(status, (uint32_t)ST_CONF_RANGE);
            }
            continue;
        }
        const float* p = post + bc * C + start;
        double s = 0.0;
        for (int k = lane; k < r.len; k += 64) s += (double)p[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);   // fixed order
        if (lane == 0) conf[i] = (float)(s / (double)r.len);
    }
}

int post_nseg(int64_t C) { return (int)((C + kSeg - 1) / kSeg); }

}  // namespace

// segment products | alpha entering | beta leaving, per segment of every chunk
size_t posterior_ws_bytes(int64_t nchunks, int64_t C) {
    const size_t n = (size_t)nchunks * (size_t)post_nseg(C);
    return n * (sizeof(Mat) + 2 * sizeof(double2)) + 256;
}

hipError_t launch_posterior(const cpg_model& model, const double2* gtab, const uint32_t* packed,
                            int64_t nchunks, int64_t C, void* ws, float* post, uint32_t* sign,
                            double* loglik, hipStream_t s) {
    if (nchunks <= 0 || C < 1 || !gtab) return hipErrorInvalidValue;
    const int nseg = post_nseg(C);
    const int64_t nblk = nchunks * nseg;
    if (nblk > 0x7FFFFFFFll) return hipErrorInvalidValue;
    // lanes of a full segment (whole waves); a chunk's last segment may leave lanes idle
    const int64_t seglen = C < kSeg ? C : kSeg;
    const int lanes = (int)(((seglen + kLanePos - 1) / kLanePos + 63) / 64 * 64);
    Mat* segP = static_cast<Mat*>(ws);
    // (sizeof(Mat) = 40: the double2 arrays start 16-byte aligned after a multiple of 2 Mats)
    double2* ain = reinterpret_cast<double2*>(
        static_cast<unsigned char*>(ws) + (((size_t)nblk * sizeof(Mat) + 15) & ~(size_t)15));
    double2* bout = ain + nblk;
    hipLaunchKernelGGL(k_post_seg, dim3((unsigned)nblk), dim3(lanes), 0, s, gtab, packed, C, nseg,
                       segP);
    hipLaunchKernelGGL(k_post_scan, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0, s,
                       model, packed, nchunks, C, nseg, segP, ain, bout, loglik);
    if (post || sign) {
        const size_t lds = 2048 + (post ? (size_t)(lanes / 64) * kStageWave * sizeof(float) : 0);
        if (post && sign)
            hipLaunchKernelGGL((k_post_emit<true, true>), dim3((unsigned)nblk), dim3(lanes), lds,
                               s, gtab, packed, C, nseg, ain, bout, post, sign);
        else if (post)
            hipLaunchKernelGGL((k_post_emit<true, false>), dim3((unsigned)nblk), dim3(lanes), lds,
                               s, gtab, packed, C, nseg, ain, bout, post, sign);
        else
            hipLaunchKernelGGL((k_post_emit<false, true>), dim3((unsigned)nblk), dim3(lanes), lds,
                               s, gtab, packed, C, nseg, ain, bout, post, sign);
    }
    return hipGetLastError();
}

hipError_t launch_island_conf(const float* post, int64_t nchunks, int64_t C, int64_t first_chunk,
                              const cpg_island* isl, const int64_t* count, int64_t cap,
                              float* conf, uint32_t* status, hipStream_t s) {
    if (cap <= 0) return hipSuccess;
    const int64_t blocks = (cap + 3) / 4;   // 4 waves per workgroup, one record per wave and turn
    hipLaunchKernelGGL(k_island_conf, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256),
                       0, s, post, nchunks, C, first_chunk, isl, count, cap, conf, status);
    return hipGetLastError();
}

}  // namespace cpg
