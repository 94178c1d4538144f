// The Lagrange-basis commitment key: a number-theoretic transform whose ELEMENTS are points of the curve of the ctx's field (h2r_curve.hpp;
// today bn256 G1) and whose twiddle products are scalar multiplications.  DESIGN.md section 2k.  With n = 2^log_n, natural order both sides:
//   forward  out[i] = sum_j [w^(i j)] in[j]          inverse  out[i] = [n^-1] sum_j [w^(-i j)] in[j]
// (halo2's g_to_lagrange is the inverse transform of the first n points of g; restated, not pinned).
// The points live as projective triples of CNTT_POINT_BYTES in the workspace; radix 2, decimation in time, in place:
//   curve_ntt_twiddle_kernel   tw[t] = w^t for t < n / 2 as CANONICAL integers (one conversion per twiddle, never per bit)
//   curve_ntt_load_kernel      pts[bitrev(j)] = in[j] (affine -> projective; (0, 0) -> (0 : 1 : 0); a canonical ctx converts here)
//   curve_ntt_stage_kernel     stage s = 1 .. log_n, one launch each: the lane owns the pair (i, i + 2^(s-1)) of the group of 2^s:
//                              v = [tw] pts[i + half]; pts[i] = u + v; pts[i + half] = u - v
//   curve_ntt_store_kernel     out[i] = affine([n^-1] pts[i]) (the multiplication only for the inverse), canonical representatives
// No workgroup waits for another, no atomics, every loop has a fixed trip count; a launch is sliced by blocks (a.block0).
// THE SCALAR MULTIPLICATION decides the run time (a butterfly is one of them plus two additions).  Stage s has 2^(s-1) distinct twiddles
// and n / 2^s butterflies per twiddle.  Where that is >= CNTT_UNIFORM_MIN_GROUPS = 64 = a wavefront, the lanes are numbered twiddle-major,
// every wave holds butterflies of ONE twiddle, and pt_mul_uniform runs double-and-add over the twiddle's non-adjacent form: the digits sit
// in scalar registers, the branches are uniform, a zero digit (two of three) costs only its doubling.  In the last six stages (and everywhere for n < 128)
// the lanes are numbered group-major and hold different twiddles: pt_mul_window2 walks fixed 2-bit windows with the lane's table
// {O, P, 2P, 3P}, selected by masks; adding O runs through algorithm 7 like anything else, so no window branches.  Twiddle w^0 = 1 (all of
// stage 1, one butterfly per group later) skips the multiplication: a uniform branch in the twiddle-major stages, a divergent one elsewhere.
// Both forms take any 256-bit integer (256 bits / 128 windows: fixed trip counts); h2r_curve_eval ops 6 and 7 run them on the host.
#pragma once

#include "h2r_curve.hpp"
#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 CNTT_MAX_LOG = 24;
constexpr u32 CNTT_POINT_BYTES = 96;              // a projective point
constexpr u32 CNTT_UNIFORM_MIN_GROUPS = 64;       // butterflies per twiddle from which a stage is numbered twiddle-major (a wavefront)
constexpr u32 CNTT_FORM_DEFAULT = 0, CNTT_FORM_PER_LANE = 1;   // per-lane bit-by-bit double-and-add everywhere: the timing tool's baseline, -DH2R_DEV_KNOBS builds only

struct CurveNttArgs {
    const u8 *in;                   // [n][2][4] u64, the ctx's representation
    u8 *out;                        // likewise
    u8 *pts;                        // [n] projective points (workspace)
    u64 *tw;                        // [n / 2][4] canonical twiddles (workspace)
    u32 log_n, stage, mont, inverse, block0, form, pad_[2];
    Fe wpow[CNTT_MAX_LOG];          // w^(2^b), Montgomery form of the scalar field (w = omega or omega^-1)
    u64 ninv[4];                    // n^-1 mod r, canonical
    FieldConsts fr;                 // the scalars' field (the ctx's)
    CurveConsts cv;
};

__host__ __device__ inline u64 curve_ntt_workspace_bytes(u32 log_n) { return 256 + ((u64)CNTT_POINT_BYTES << log_n) + ((u64)16 << log_n); }

H2R_FD PtProj pt_neg(const PtProj &p, const CurveConsts &c) { PtProj r = p; r.y = fe_sub(fe_zero(), p.y, c.fq.p); return r; }

// [k]P for a k every lane of the wave shares: the non-adjacent form of k from the top, one doubling per digit and one complete addition of
// P or -P per NON-ZERO digit (a third of them on average; a zero digit costs a uniform branch).  With h = 3 k, digit i of the form is
// bit(h, i + 1) - bit(k, i + 1), so the digits +1 are the bits of (h & ~k) >> 1 and the digits -1 those of (~h & k) >> 1: digits 0 .. 256 for
// any 256-bit k, the top one never negative.  The masks are shifted out of their top words: no indexed access, 256 trips whatever k is.
H2R_FD PtProj pt_mul_uniform(const PtProj &p, const u64 (&k)[4], const CurveConsts &c) {
    u64 h[5], cy = 0;
    const u64 d[5] = {k[0] << 1, (k[1] << 1) | (k[0] >> 63), (k[2] << 1) | (k[1] >> 63), (k[3] << 1) | (k[2] >> 63), k[3] >> 63};
    const u64 kk[5] = {k[0], k[1], k[2], k[3], 0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 5; ++i) { const u64 t = kk[i] + d[i]; const u64 c1 = t < kk[i]; h[i] = t + cy; cy = c1 | (u64)(h[i] < t); }
    u64 pos[4], neg[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        pos[i] = ((h[i] & ~kk[i]) >> 1) | ((h[i + 1] & ~kk[i + 1]) << 63);
        neg[i] = ((~h[i] & kk[i]) >> 1) | ((~h[i + 1] & kk[i + 1]) << 63);
    }
    u64 p0 = pos[0], p1 = pos[1], p2 = pos[2], p3 = pos[3], n0 = neg[0], n1 = neg[1], n2 = neg[2], n3 = neg[3];
    const PtProj np = pt_neg(p, c);
    PtProj acc = pt_identity(c);
    if ((h[4] >> 1) & 1u) acc = p;                          // digit 256
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int bit = 0; bit < 256; ++bit) {
        acc = pt_double(acc, c);
        if (p3 >> 63) acc = pt_add(acc, p, c);
        else if (n3 >> 63) acc = pt_add(acc, np, c);
        p3 = (p3 << 1) | (p2 >> 63); p2 = (p2 << 1) | (p1 >> 63); p1 = (p1 << 1) | (p0 >> 63); p0 <<= 1;
        n3 = (n3 << 1) | (n2 >> 63); n2 = (n2 << 1) | (n1 >> 63); n1 = (n1 << 1) | (n0 >> 63); n0 <<= 1;
    }
    return acc;
}
#ifdef H2R_DEV_KNOBS
// [k]P by plain bit-by-bit double-and-add from the top of 256 bits: what a lane with a twiddle of its own would run without windows.  Only
// the timing tool's baseline (CNTT_FORM_PER_LANE) runs it; the product library does not contain it.
H2R_FD PtProj pt_mul_binary(const PtProj &p, const u64 (&k)[4], const CurveConsts &c) {
    u64 k0 = k[0], k1 = k[1], k2 = k[2], k3 = k[3];
    PtProj acc = pt_identity(c);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int bit = 0; bit < 256; ++bit) {
        acc = pt_double(acc, c);
        if (k3 >> 63) acc = pt_add(acc, p, c);
        k3 = (k3 << 1) | (k2 >> 63); k2 = (k2 << 1) | (k1 >> 63); k1 = (k1 << 1) | (k0 >> 63); k0 <<= 1;
    }
    return acc;
}
#endif

// the window's multiple out of {O, P, 2P, 3P} by masks: no branch, no indexed registers
H2R_FD Fe fe_select4(u32 d, const Fe &e0, const Fe &e1, const Fe &e2, const Fe &e3) {
    const u64 m0 = 0 - (u64)(d == 0u), m1 = 0 - (u64)(d == 1u), m2 = 0 - (u64)(d == 2u), m3 = 0 - (u64)(d == 3u);
    Fe r;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) r.v[i] = (e0.v[i] & m0) | (e1.v[i] & m1) | (e2.v[i] & m2) | (e3.v[i] & m3);
    return r;
}
// [k]P for a k of the lane's own: 128 fixed windows of 2 bits from the top, two doublings and one complete addition each
H2R_FD PtProj pt_mul_window2(const PtProj &p, const u64 (&k)[4], const CurveConsts &c) {
    u64 k0 = k[0], k1 = k[1], k2 = k[2], k3 = k[3];
    const PtProj o = pt_identity(c), p2 = pt_double(p, c), p3 = pt_add(p2, p, c);
    PtProj acc = o;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int w = 0; w < 128; ++w) {
        acc = pt_double(pt_double(acc, c), c);
        const u32 d = (u32)(k3 >> 62);
        PtProj t;
        t.x = fe_select4(d, o.x, p.x, p2.x, p3.x); t.y = fe_select4(d, o.y, p.y, p2.y, p3.y); t.z = fe_select4(d, o.z, p.z, p2.z, p3.z);
        acc = pt_add(acc, t, c);
        k3 = (k3 << 2) | (k2 >> 62); k2 = (k2 << 2) | (k1 >> 62); k1 = (k1 << 2) | (k0 >> 62); k0 <<= 2;
    }
    return acc;
}

#ifdef H2R_TU_CURVE_NTT

// grid (blocks of 256 over n / 2 twiddles): tw[t] = w^t, the product of the squaring chain's entries at t's bits, as a canonical integer
__global__ __launch_bounds__(256) void curve_ntt_twiddle_kernel(CurveNttArgs a) {
    const u64 t = ((u64)a.block0 + blockIdx.x) * 256 + threadIdx.x;
    if (t >= (1ull << (a.log_n - 1))) return;
    Fe acc = fe_load_one(a.fr);
#pragma unroll
    for (u32 b = 0; b < CNTT_MAX_LOG - 1; ++b)
        if ((t >> b) & 1u) acc = fe_mont_mul(acc, a.wpow[b], a.fr);
    acc = fe_from_mont(acc, a.fr);
    fe_store(reinterpret_cast<u8 *>(a.tw + 4 * t), acc);
}

// grid (blocks of 256 over n points)
__global__ __launch_bounds__(256) void curve_ntt_load_kernel(CurveNttArgs a) {
    const u64 j = ((u64)a.block0 + blockIdx.x) * 256 + threadIdx.x;
    if (j >= (1ull << a.log_n)) return;
    PtProj p;
    p.x = fe_load(a.in + j * 64); p.y = fe_load(a.in + j * 64 + 32);
    if (fe_is_zero(p.x) && fe_is_zero(p.y)) p = pt_identity(a.cv);
    else {
        if (!a.mont) { p.x = fe_to_mont(p.x, a.cv.fq); p.y = fe_to_mont(p.y, a.cv.fq); }
        p.z = fe_load_one(a.cv.fq);
    }
    const u64 r = (u64)(__brev((u32)j) >> (32 - a.log_n));
    pt_store(a.pts + r * CNTT_POINT_BYTES, p);
}

// grid (blocks of 256 over n / 2 butterflies), stage a.stage = 1 .. log_n
__global__ __launch_bounds__(256) void curve_ntt_stage_kernel(CurveNttArgs a) {
    const u64 t = ((u64)a.block0 + blockIdx.x) * 256 + threadIdx.x;
    if (t >= (1ull << (a.log_n - 1))) return;
    const u32 s = a.stage, log_groups = a.log_n - s;       // half = 2^(s-1) twiddles, 2^log_groups butterflies each
    const u64 half = 1ull << (s - 1);
    const bool twiddle_major = (1ull << log_groups) >= CNTT_UNIFORM_MIN_GROUPS;
    u64 k, g;
    if (twiddle_major) { k = t >> log_groups; g = t & ((1ull << log_groups) - 1); }
    else { k = t & (half - 1); g = t >> (s - 1); }
    u8 *lo = a.pts + ((g << s) + k) * CNTT_POINT_BYTES, *hi = lo + half * CNTT_POINT_BYTES;
    PtProj v = pt_load(hi);
#ifdef H2R_DEV_KNOBS
    if (a.form == CNTT_FORM_PER_LANE) {
        if (k) {
            const Fe w = fe_load(reinterpret_cast<const u8 *>(a.tw + 4 * (k << log_groups)));
            v = pt_mul_binary(v, w.v, a.cv);
        }
    } else
#endif
    if (twiddle_major) {
        // 64 consecutive t share k (2^log_groups is a multiple of the wavefront): the twiddle is read through scalar registers
        const u32 ku = __builtin_amdgcn_readfirstlane((u32)k);
        if (ku) {
            const u64 *w = a.tw + 4 * ((u64)ku << log_groups);
            const u64 kk[4] = {w[0], w[1], w[2], w[3]};
            v = pt_mul_uniform(v, kk, a.cv);
        }
    } else if (k) {
        const Fe w = fe_load(reinterpret_cast<const u8 *>(a.tw + 4 * (k << log_groups)));
        v = pt_mul_window2(v, w.v, a.cv);
    }
    const PtProj u = pt_load(lo);
    pt_store(lo, pt_add(u, v, a.cv));
    pt_store(hi, pt_add(u, pt_neg(v, a.cv), a.cv));
}

// grid (blocks of 256 over n points)
__global__ __launch_bounds__(256) void curve_ntt_store_kernel(CurveNttArgs a) {
    const u64 i = ((u64)a.block0 + blockIdx.x) * 256 + threadIdx.x;
    if (i >= (1ull << a.log_n)) return;
    PtProj p = pt_load(a.pts + i * CNTT_POINT_BYTES);
    if (a.inverse) p = pt_mul_uniform(p, a.ninv, a.cv);    // (n^-1 is the same for every lane of the call)
    PtAff r = pt_to_affine(p, a.cv);
    if (!a.mont) { r.x = fe_from_mont(r.x, a.cv.fq); r.y = fe_from_mont(r.y, a.cv.fq); }
    fe_store(a.out + i * 64, r.x); fe_store(a.out + i * 64 + 32, r.y);
}

#endif  // H2R_TU_CURVE_NTT

}  // namespace h2r
