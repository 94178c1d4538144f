// The Fiat-Shamir transcript of halo2's create_proof: Blake2bWrite<_, G1Affine, Challenge255<_>> over the curve of the ctx's field
// (h2r_curve.hpp; today bn256 G1 for H2R_FIELD_BN254_FR), for a batch of circuits.  DESIGN.md section 2l.
// THE HASH is BLAKE2b (RFC 7693) with a 64-byte digest, no key, no salt and the 16-byte personalisation "Halo2-Transcript".  The state
// is STREAMING: bytes gather in a 128-byte block, and a full block is compressed only when more input arrives, because the last block
// of a message carries the final flag.  A squeeze absorbs the byte 0x00, finalises a COPY of the state (the running state keeps the
// 0x00 and goes on), reads the 64 digest bytes as a little-endian 512-bit integer and reduces it modulo r.
// THE FRAMING (a restatement of halo2 and halo2curves, not pinned against them): a point absorbs 0x01, x, y; a scalar absorbs 0x02 and
// its value; every field element as its 32 little-endian canonical bytes.  A written scalar is those 32 bytes, a written point the 32
// bytes of x with bit 7 of byte 31 set to the lowest bit of canonical y.  The point at infinity, (0, 0), cannot be absorbed.
// Host and device share every formula (H2R_FD): h2r_transcript_eval runs on the host exactly what the kernel inlines.  The 128-byte
// block is reached through TrBlock (word i at w[i * stride]): a plain array on the host, the lane's column of a lane-interleaved LDS
// tile on the device, where items arrive in pieces of 33 and 65 bytes at arbitrary block offsets and a register array indexed by a
// run-time byte offset would spill.  The compression function is fully unrolled with the message permutation as compile-time indices;
// it has ONE call site per absorbing loop (tr_absorb flushes at one place), so a kernel carries three copies of it, not one per word.
// transcript_kernel: one launch per round, one lane per circuit, 64 circuits per workgroup; no workgroup waits for another, no atomics,
// no barrier (a lane touches only its own LDS column).  The batch is the parallel axis; a lane's chain of compressions is the latency.
#pragma once

#include "h2r_curve.hpp"
#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 TR_MAX_ITEMS = 64, TR_MAX_SQUEEZE = 8, TR_MAX_DERIVE = 16, TR_MAX_COUNT = 1u << 16, TR_MAX_LOG2_POW = 24;
constexpr u32 TR_POINT = 1, TR_SCALAR = 2, TR_COMMON = 1;
constexpr u32 TR_LANES = 64;                       // circuits of a workgroup: one wavefront
// A circuit's running state in memory, 16-byte aligned: words 0..7 = h, 8 = bytes compressed so far, 9 = fill of the block, 10..25 = the block
constexpr u32 TR_STATE_WORDS = 26, TR_STATE_BYTES = TR_STATE_WORDS * 8, TR_W_T = 8, TR_W_FILL = 9, TR_W_BLOCK = 10;

struct TrBlock { u64 *w; u32 stride; };
H2R_FD u64 tr_get(const TrBlock &b, u32 i) { return b.w[i * b.stride]; }
H2R_FD void tr_set(const TrBlock &b, u32 i, u64 v) { b.w[i * b.stride] = v; }
struct TrHash { u64 h[8]; u64 t; u32 fill; };
// the scalars' field, the coordinates' field, R^3 mod r (the wide reduction), whether the ctx's representation is the Montgomery form
struct TrConsts { FieldConsts fr, fq; u64 r3[4]; u32 mont, pad_; };

// RFC 7693 section 2.7: the message word schedule (rounds 10 and 11 repeat rows 0 and 1)
constexpr uint8_t kB2Sigma[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

H2R_FD u64 b2_rotr(u64 x, int n) { return (x >> n) | (x << (64 - n)); }
H2R_FD void b2_g(u64 &a, u64 &b, u64 &c, u64 &d, u64 x, u64 y) {
    a = a + b + x; d = b2_rotr(d ^ a, 32); c = c + d; b = b2_rotr(b ^ c, 24);
    a = a + b + y; d = b2_rotr(d ^ a, 16); c = c + d; b = b2_rotr(b ^ c, 63);
}
template <int R> H2R_FD void b2_round(u64 (&v)[16], const u64 (&m)[16]) {
    constexpr int S = R % 10;
    b2_g(v[0], v[4], v[8], v[12], m[kB2Sigma[S][0]], m[kB2Sigma[S][1]]);
    b2_g(v[1], v[5], v[9], v[13], m[kB2Sigma[S][2]], m[kB2Sigma[S][3]]);
    b2_g(v[2], v[6], v[10], v[14], m[kB2Sigma[S][4]], m[kB2Sigma[S][5]]);
    b2_g(v[3], v[7], v[11], v[15], m[kB2Sigma[S][6]], m[kB2Sigma[S][7]]);
    b2_g(v[0], v[5], v[10], v[15], m[kB2Sigma[S][8]], m[kB2Sigma[S][9]]);
    b2_g(v[1], v[6], v[11], v[12], m[kB2Sigma[S][10]], m[kB2Sigma[S][11]]);
    b2_g(v[2], v[7], v[8], v[13], m[kB2Sigma[S][12]], m[kB2Sigma[S][13]]);
    b2_g(v[3], v[4], v[9], v[14], m[kB2Sigma[S][14]], m[kB2Sigma[S][15]]);
}
// h <- F(h, block, t, last): the block's first `nwords` words are message, the rest count as zero (a last block is padded with zeros);
// t = the bytes of the message up to and including this block
H2R_FD void tr_compress(u64 (&h)[8], const TrBlock &blk, u32 nwords, u64 t, bool last) {
    u64 m[16], v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = (u32)i < nwords ? tr_get(blk, i) : 0ull;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = h[i];
    v[8] = 0x6a09e667f3bcc908ull; v[9] = 0xbb67ae8584caa73bull; v[10] = 0x3c6ef372fe94f82bull; v[11] = 0xa54ff53a5f1d36f1ull;
    v[12] = 0x510e527fade682d1ull ^ t; v[13] = 0x9b05688c2b3e6c1full;   // (the counter's high word: a transcript stays far below 2^64 bytes)
    v[14] = last ? ~0x1f83d9abfb41bd6bull : 0x1f83d9abfb41bd6bull; v[15] = 0x5be0cd19137e2179ull;
    b2_round<0>(v, m); b2_round<1>(v, m); b2_round<2>(v, m); b2_round<3>(v, m); b2_round<4>(v, m); b2_round<5>(v, m);
    b2_round<6>(v, m); b2_round<7>(v, m); b2_round<8>(v, m); b2_round<9>(v, m); b2_round<10>(v, m); b2_round<11>(v, m);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}
// the empty transcript: IV ^ the parameter block (digest 64, no key, fanout 1, depth 1; no salt; the personalisation in words 6 and 7)
H2R_FD void tr_init(TrHash &s) {
    s.h[0] = 0x6a09e667f3bcc908ull ^ 0x01010040ull; s.h[1] = 0xbb67ae8584caa73bull; s.h[2] = 0x3c6ef372fe94f82bull; s.h[3] = 0xa54ff53a5f1d36f1ull;
    s.h[4] = 0x510e527fade682d1ull; s.h[5] = 0x9b05688c2b3e6c1full;
    s.h[6] = 0x1f83d9abfb41bd6bull ^ 0x72542d326f6c6148ull;   // "Halo2-Tr"
    s.h[7] = 0x5be0cd19137e2179ull ^ 0x7470697263736e61ull;   // "anscript"
    s.t = 0; s.fill = 0;
}
// the n <= 8 low bytes of v (its other bytes zero) join the message.  Invariant: in the block's word that holds byte `fill` the bytes
// from `fill` on are zero.  The ONE flush: a full block is compressed here, when the next byte arrives, never before.
H2R_FD void tr_absorb(TrHash &s, const TrBlock &blk, u64 v, u32 n) {
    const u32 sh = s.fill & 7u;
    u32 taken = 0;
    if (s.fill < 128) {
        const u32 w = s.fill >> 3;
        tr_set(blk, w, sh ? tr_get(blk, w) | (v << (8 * sh)) : v);
        taken = n < 8 - sh ? n : 8 - sh;
    }
    if (taken < n) {   // the rest starts a word (taken < 8 here: no shift by 64)
        u32 w = (s.fill + taken) >> 3;
        if (w == 16) { tr_compress(s.h, blk, 16, s.t + 128, false); s.t += 128; s.fill -= 128; w = 0; }
        tr_set(blk, w, v >> (8 * taken));
    }
    s.fill += n;
}
// prefix byte, then the elements' canonical words: a point is 9 pieces (x, y), a scalar 5 (x alone)
H2R_FD void tr_absorb_item(TrHash &s, const TrBlock &blk, u32 kind, const Fe &x, const Fe &y) {
    const u32 pieces = kind == TR_POINT ? 9u : 5u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (u32 c = 0; c < pieces; ++c) {
        const u64 v = c == 0 ? (u64)kind : c == 1 ? x.v[0] : c == 2 ? x.v[1] : c == 3 ? x.v[2] : c == 4 ? x.v[3]
                    : c == 5 ? y.v[0] : c == 6 ? y.v[1] : c == 7 ? y.v[2] : y.v[3];
        tr_absorb(s, blk, v, c == 0 ? 1u : 8u);
    }
}
// the digest of the message so far: a copy of h is finalised, the running state is not touched
H2R_FD void tr_digest(const TrHash &s, const TrBlock &blk, u64 (&d)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = s.h[i];
    tr_compress(d, blk, (s.fill + 7) >> 3, s.t + s.fill, true);
}
// The digest as a little-endian 512-bit integer d0 + 2^256 d1, modulo r, in Montgomery form: d0 R^2 + d1 R^3 under fe_mont_mul.  Either
// half is >= r in most draws.  fe_mont_mul(a, b) takes b one word at a time and keeps its accumulator below a + p after every word
// whatever that word is, so for a < p and ANY 256-bit b the value before the conditional subtraction is below 2 p and the result is
// the reduced product: the digest half goes SECOND, the constant first.
H2R_FD Fe tr_reduce_wide(const u64 (&d)[8], const TrConsts &c) {
    Fe d0, d1;
#pragma unroll
    for (int k = 0; k < 4; ++k) { d0.v[k] = d[k]; d1.v[k] = d[k + 4]; }
    return fe_add(fe_mont_mul(fe_words(c.fr.r2), d0, c.fr), fe_mont_mul(fe_words(c.r3), d1, c.fr), c.fr.p);
}
// one squeeze: the challenge in Montgomery form
H2R_FD Fe tr_squeeze(TrHash &s, const TrBlock &blk, const TrConsts &c) {
    tr_absorb(s, blk, 0, 1);
    u64 d[8];
    tr_digest(s, blk, d);
    return tr_reduce_wide(d, c);
}
// mult * c^(2^log2_pow), everything in Montgomery form
H2R_FD Fe tr_derive(Fe c, const Fe &mult, u32 log2_pow, const FieldConsts &fr) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (u32 l = 0; l < log2_pow; ++l) c = fe_mont_mul(c, c, fr);
    return fe_mont_mul(c, mult, fr);
}
// an element of the ctx's representation: its status (0, H2R_E_SHAPE for a value >= the modulus; for a point H2R_E_ASSERTION for (0, 0))
H2R_FD u32 tr_check_item(u32 kind, const Fe &x, const Fe &y, const TrConsts &c) {
    if (kind == TR_POINT) {
        if (ge_p(x.v, c.fq.p) || ge_p(y.v, c.fq.p)) return (u32)H2R_E_SHAPE;
        return fe_is_zero(x) && fe_is_zero(y) ? (u32)H2R_E_ASSERTION : 0u;
    }
    return ge_p(x.v, c.fr.p) ? (u32)H2R_E_SHAPE : 0u;
}
// ... to canonical integers (one conversion per coordinate or scalar in a Montgomery ctx)
H2R_FD void tr_canonical(u32 kind, Fe &x, Fe &y, const TrConsts &c) {
    if (!c.mont) return;
    if (kind == TR_POINT) { x = fe_from_mont(x, c.fq); y = fe_from_mont(y, c.fq); }
    else x = fe_from_mont(x, c.fr);
}
// the 32 proof bytes of a canonical item: the scalar itself; x with the top bit carrying y's parity
H2R_FD Fe tr_encode(u32 kind, const Fe &x, const Fe &y) {
    Fe r = x;
    if (kind == TR_POINT) r.v[3] |= (y.v[0] & 1ull) << 63;
    return r;
}
H2R_FD Fe tr_to_repr(const Fe &m, const TrConsts &c) { return c.mont ? m : fe_from_mont(m, c.fr); }   // Montgomery form -> the ctx's representation

struct TrItem { const u8 *base; u64 elem_stride; u32 count, kind_flags; };   // kind | flags << 8
struct TrDerive { u64 mult[4]; u32 src, log2_pow; };                           // mult in Montgomery form
struct TranscriptArgs {
    TrItem items[TR_MAX_ITEMS];
    TrDerive derive[TR_MAX_DERIVE];
    u8 *states;                     // [batch][TR_STATE_BYTES]
    u64 *challenges;                // [batch][num_squeeze][4]
    u64 *derived;                   // [batch][num_derive][4]
    u8 *proof;                      // circuit e writes at proof + e * proof_stride + proof_off
    u8 *status;                     // nullable, never cleared
    u64 proof_stride, proof_off, batch;
    u32 num_items, num_squeeze, num_derive, init, block0, pad_;
    TrConsts c;
};

#ifdef H2R_TU_TRANSCRIPT

// grid (workgroups of one launch), 64 lanes: lane l of workgroup b is circuit (block0 + b) * 64 + l
__global__ __launch_bounds__(TR_LANES) void transcript_kernel(TranscriptArgs a) {
    __shared__ u64 tile[16 * TR_LANES];   // word i of lane l at tile[i * 64 + l]: the 64 lanes of a wave read 64 consecutive words
    const u32 lane = threadIdx.x;
    const u64 e = ((u64)a.block0 + blockIdx.x) * TR_LANES + lane;
    if (e >= a.batch) return;
    if (a.status && a.status[e]) return;                  // nonzero on entry: skipped, nothing is written
    // first every item is checked: a circuit that gets a status leaves its state, its proof bytes and its outputs as they were
    u32 bad = 0;
#pragma unroll 1
    for (u32 i = 0; i < a.num_items && !bad; ++i) {
        const TrItem it = a.items[i];
        const u32 kind = it.kind_flags & 0xffu, size = kind == TR_POINT ? 64u : 32u;
        const u8 *p = it.base + e * it.elem_stride;
#pragma unroll 1
        for (u32 k = 0; k < it.count && !bad; ++k, p += size) {
            const Fe x = fe_load(p), y = kind == TR_POINT ? fe_load(p + 32) : fe_zero();
            bad = tr_check_item(kind, x, y, a.c);
        }
    }
    if (bad) { if (a.status) a.status[e] = (u8)bad; return; }

    const TrBlock blk{tile + lane, TR_LANES};
    TrHash s;
    u64 *sp = reinterpret_cast<u64 *>(a.states + e * TR_STATE_BYTES);
    if (a.init) {
        tr_init(s);
#pragma unroll
        for (int i = 0; i < 16; ++i) tr_set(blk, i, 0);
    } else {
#pragma unroll
        for (int i = 0; i < (int)TR_STATE_WORDS; i += 2) {
            const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(sp + i);
            if (i < 8) { s.h[i] = q.x; s.h[i + 1] = q.y; }
            else if (i == 8) { s.t = q.x; s.fill = q.y < 128 ? (u32)q.y : 128u; }   // (a record nobody initialised indexes nothing out of the tile)
            else { tr_set(blk, i - TR_W_BLOCK, q.x); tr_set(blk, i + 1 - TR_W_BLOCK, q.y); }
        }
    }
    u8 *pw = a.proof + e * a.proof_stride + a.proof_off;   // (dereferenced only for a written item: the host refuses a null proof then)
#pragma unroll 1
    for (u32 i = 0; i < a.num_items; ++i) {
        const TrItem it = a.items[i];
        const u32 kind = it.kind_flags & 0xffu, size = kind == TR_POINT ? 64u : 32u;
        const bool written = !((it.kind_flags >> 8) & TR_COMMON);
        const u8 *p = it.base + e * it.elem_stride;
        // (loading the next entry while this one is hashed was measured and changes nothing: the chain of compressions is the latency)
#pragma unroll 1
        for (u32 k = 0; k < it.count; ++k, p += size) {
            Fe x = fe_load(p), y = kind == TR_POINT ? fe_load(p + 32) : fe_zero();
            tr_canonical(kind, x, y, a.c);
            tr_absorb_item(s, blk, kind, x, y);
            if (written) { fe_store(pw, tr_encode(kind, x, y)); pw += 32; }
        }
    }
    u8 *ch = reinterpret_cast<u8 *>(a.challenges) + e * a.num_squeeze * 32;
#pragma unroll 1
    for (u32 k = 0; k < a.num_squeeze; ++k) fe_store(ch + k * 32, tr_to_repr(tr_squeeze(s, blk, a.c), a.c));
    u8 *dv = reinterpret_cast<u8 *>(a.derived) + e * a.num_derive * 32;
#pragma unroll 1
    for (u32 j = 0; j < a.num_derive; ++j) {
        const TrDerive d = a.derive[j];
        const Fe c = fe_load_mont(ch + d.src * 32, a.c.mont, a.c.fr);   // this lane's own store of a moment ago
        fe_store(dv + j * 32, tr_to_repr(tr_derive(c, fe_words(d.mult), d.log2_pow, a.c.fr), a.c));
    }
#pragma unroll
    for (int i = 0; i < (int)TR_STATE_WORDS; i += 2) {
        ulonglong2 q;
        if (i < 8) q = make_ulonglong2(s.h[i], s.h[i + 1]);
        else if (i == 8) q = make_ulonglong2(s.t, (u64)s.fill);
        else q = make_ulonglong2(tr_get(blk, i - TR_W_BLOCK), tr_get(blk, i + 1 - TR_W_BLOCK));
        *reinterpret_cast<ulonglong2 *>(sp + i) = q;
    }
}

#endif  // H2R_TU_TRANSCRIPT

}  // namespace h2r
