// The prover's randomness on the device: the blinding rows of the advice, A', S' and Z columns and the vanishing argument's random
// polynomial, as a COUNTER-BASED generator.  DESIGN.md section 2m.  Every element is a pure function of (seed, circuit, tag, row):
//     element = reduce_wide( BLAKE2b-512( person = "H2R-Blinding-v1\0", msg = seed[32] | le64(circuit) | le32(tag) | le32(0) | le64(row) ) )
// so that a proof is reproducible from its seed, the result does not depend on how a batch or a row range is cut into launches, and
// Python's hashlib is a true oracle (tests/create_proof_ref.py).  The message is 56 bytes: ONE compression per element, a last block of
// seven words.  reduce_wide is tr_reduce_wide: the 64 digest bytes as a little-endian 512-bit integer modulo r, as Challenge255 and
// Fr::random's from_bytes_wide do it; the value is stored in the ctx's representation, so one seed gives one VALUE on a canonical and
// on a Montgomery ctx.  There is no second BLAKE2b in the tree: tr_compress and tr_reduce_wide of h2r_transcript.hpp do the work, the
// message reaches them through a TrBlock over seven words of the caller's -- a plain array, on the host and on the device alike -- and
// h2r_random_eval runs on the host exactly what the kernel inlines (H2R_FD).  transcript_kernel stages its block in LDS because items
// land at run-time byte offsets; here every index into the block is a compile-time constant, so the seven words are registers (like
// tr_compress's own m[16] and v[16]) and the kernel uses no LDS.
// random_kernel: one lane per element, 256 consecutive rows of one column of one circuit per workgroup, grid (row tile, column,
// circuit): one launch serves the six-row tails of thirty columns and a whole 2^17-row column alike.  Adjacent lanes take adjacent
// rows, so a wavefront stores 2 KB contiguous.  No LDS, no barrier, no atomics, no scratch, no workgroup waits for another.  The seed
// travels in the kernel arguments.
#pragma once

#include "h2r_transcript.hpp"

namespace h2r {

constexpr u32 RND_MAX_COLUMNS = 64, RND_LANES = 256, RND_MSG_WORDS = 7, RND_MSG_BYTES = 8 * RND_MSG_WORDS;
constexpr u64 RND_MAX_ROW = 1ull << 58;   // row * 32 stays far inside 64 bits

// IV ^ the parameter block (digest 64, no key, fanout 1, depth 1; no salt; the personalisation in words 6 and 7)
H2R_FD void rnd_init(u64 (&h)[8]) {
    h[0] = 0x6a09e667f3bcc908ull ^ 0x01010040ull; h[1] = 0xbb67ae8584caa73bull; h[2] = 0x3c6ef372fe94f82bull; h[3] = 0xa54ff53a5f1d36f1ull;
    h[4] = 0x510e527fade682d1ull; h[5] = 0x9b05688c2b3e6c1full;
    h[6] = 0x1f83d9abfb41bd6bull ^ 0x6e696c422d523248ull;   // "H2R-Blin"
    h[7] = 0x5be0cd19137e2179ull ^ 0x0031762d676e6964ull;   // "ding-v1\0"
}
// one element in the ctx's representation; blk: seven words of the caller's, overwritten
H2R_FD Fe rnd_element(const u64 (&seed)[4], u64 circuit, u32 tag, u64 row, const TrBlock &blk, const TrConsts &c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) tr_set(blk, k, seed[k]);
    tr_set(blk, 4, circuit); tr_set(blk, 5, (u64)tag); tr_set(blk, 6, row);
    u64 h[8];
    rnd_init(h);
    tr_compress(h, blk, RND_MSG_WORDS, RND_MSG_BYTES, true);
    return tr_to_repr(tr_reduce_wide(h, c), c);
}

struct RndColumn { u8 *base; u64 elem_stride; u32 tag, pad_; };
struct RandomArgs {
    RndColumn cols[RND_MAX_COLUMNS];
    u64 seed[4];                    // the 32 seed bytes as little-endian words
    u64 row_begin, row_count;       // rows [row_begin, row_begin + row_count)
    u64 first_circuit, elem0;       // circuit e of the batch draws with index first_circuit + e; blockIdx.z = e - elem0
    u64 tile0;                      // blockIdx.x = row tile - tile0
    TrConsts c;
};

#ifdef H2R_TU_RANDOM

// grid (row tiles, columns, circuits) of one launch, 256 lanes: lane l of tile t is row row_begin + t * 256 + l
__global__ __launch_bounds__(RND_LANES) void random_kernel(RandomArgs a) {
    const u32 lane = threadIdx.x;
    const u64 off = (a.tile0 + blockIdx.x) * RND_LANES + lane;
    if (off >= a.row_count) return;
    const RndColumn col = a.cols[blockIdx.y];
    const u64 e = a.elem0 + blockIdx.z;
    if (col.elem_stride == 0 && e != 0) return;       // a shared column is drawn once, as circuit first_circuit
    const u64 row = a.row_begin + off;
    u64 block[RND_MSG_WORDS];                          // constant indices only: registers
    const Fe x = rnd_element(a.seed, a.first_circuit + e, col.tag, row, TrBlock{block, 1}, a.c);
    fe_store(col.base + e * col.elem_stride + row * 32, x);
}

#endif  // H2R_TU_RANDOM

}  // namespace h2r
