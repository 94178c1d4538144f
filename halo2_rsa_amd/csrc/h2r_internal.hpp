// Internal to libh2r.so: what the library's translation units share.
//
// The library is compiled as several translation units that build side by side (the device compile of the template
// kernel families is what a build costs; each family is defined, instantiated and launched in exactly one unit):
//   h2r_tu_trace.hip   trace_kernel<LW, L>         (one record per mul_mod; every supported shape)
//   h2r_tu_chain.hip   recip / key_table / chain / chain_dual / chain_wave kernels (the dependent mul_mod chain per element)
//   h2r_tu_step.hip    step_kernel<K, NW, LW, L>   (records of call k + chains of call k+1 in one launch)
//   h2r_tu_chain_keyed.hip, h2r_tu_step_keyed.hip   the same two families' builds for keyed calls (H2R_F_KEYED_MODULI)
//   h2r_tu_cells.hip   cells_kernel<LW, ABL, MONT, NWV> (the advice image directly from the operands)
//   h2r_tu_lookup_product.hip   the lookup argument's input columns and grand product (h2r_lookup_product.hpp over h2r_grand_product.hpp)
//   h2r_tu_permutation_product.hip   the permutation argument's grand product (h2r_permutation_product.hpp over h2r_grand_product.hpp)
//   h2r_tu_ntt.hip     the evaluation domain's transforms (h2r_ntt.hpp)
//   h2r_tu_quotient.hip   the vanishing argument's quotient on the extended domain (h2r_quotient.hpp)
//   h2r_tu_open.hip    the openings: evaluations at x, GWC witness polynomials, the fold of h's pieces (h2r_open.hpp)
//   h2r_tu_msm.hip     the commitments: multi-scalar multiplications over the curve of the ctx's field (h2r_msm.hpp, h2r_curve.hpp)
//   h2r_tu_curve_ntt.hip   the Lagrange-basis commitment key: the transform over the curve's points (h2r_curve_ntt.hpp, h2r_curve.hpp)
//   h2r_tu_transcript.hip   the Fiat-Shamir transcript: one round of a batch of BLAKE2b states per launch (h2r_transcript.hpp)
//   h2r_tu_random.hip  the prover's blinding values: a counter-based generator over the transcript's BLAKE2b (h2r_random.hpp)
//   h2r_tu_verify.hip  the verifier up to the pairing: proof decoder, the accumulators' scalars, the sum of terms over per-circuit bases (h2r_verify.hpp)
//   h2r_tu_pairing.hip the verifier's verdict: Miller values and final exponentiations of pairing products against prepared G2 tables (h2r_pairing.hpp)
//   h2r_tu_keygen.hip  key generation: the fixed columns of an image's row kinds, the sigma columns of its copy pairs (h2r_keygen.hpp)
//   h2r_tu_setup.hip   KZG parameters from a known tau: the fixed-base table and multiplication over G1, the scalars tau^i and l_i(tau) (h2r_setup.hpp)
//   h2r_tu_witness.hip   the witness kernels outside the mul_mod records: assert_in_field / encoded message (aux), the Fresh ops, SHA-256, the
//                      in-place audit (check, link), range decompose, key expand, mul / refresh / is_equal_muled (h2r_muled.hpp), and the
//                      arena's fill / restore kernels and the queue probe
//   h2r_tu_advice.hip  the advice image from records and programs: advice / emit / var_rows / rowprog kernels, the layout permutation, the
//                      MockProver's row / copy checks and the image's lookup histogram (h2r_rowprog.hpp, h2r_varrows.hpp, h2r_copymap.hpp, h2r_check.hpp)
//   h2r_tu_lookup.hip  the lookup argument's multiplicities and permuted columns: hist / perm kernels over the records, the per-argument
//                      histograms, the A' / S' set-up and fill (h2r_lookup.hpp)
//   h2r_api.hip        the C ABI, the ctx, the pipelines and the host twins: host code only, no kernel is defined or launched there
// The launchers below take plain values, never the ctx: `struct h2r_ctx` stays private to h2r_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdlib>
#include <cstring>

#include "h2r.h"
#include "h2r_kernels.hpp"
#include "h2r_cells.hpp"

namespace h2r {

// Developer knobs: compiled in ONLY by the -DH2R_DEV_KNOBS build (python -m halo2_rsa_amd._build <name> -DH2R_DEV_KNOBS,
// selected with H2R_LIB by the sweeps under tools/).  The product library never reads the environment: every knob
// keeps the measured default below.
struct Knobs {
    int chain_nw = 0, chain_deep = -1;          // H2R_CHAIN_NW, H2R_CHAIN_DEEP
    long chain_wave = -1;                        // H2R_CHAIN_WAVE=0|1: the one-wavefront chain for 32-digit elements (-1 = the measured default)
    long trace_dyn_lds = -1, trace_prio = -1;    // H2R_TRACE_DYN_LDS, H2R_TRACE_PRIO
    long chain_prio = -1, ablate = 0;            // H2R_CHAIN_PRIO, H2R_ABLATE (needs the -DH2R_ABLATION build)
    int pipe_stream_prio = -1;                   // H2R_PIPE_STREAM_PRIO = low (default) | normal | high  -> -1 | 0 | +1
    bool chain_timing = false;                   // H2R_CHAIN_TIMING (needs the -DH2R_CHAIN_TIMING build)
    bool pipe_serialize = false;                 // H2R_PIPE_SERIALIZE=1: with two record streams, a record kernel also waits for the previous one
    long plain_overlap = -1;                     // H2R_PLAIN_OVERLAP=0: the plain pow exports never overlap their sub-batches internally
    long arena_chunk_mb = 0;                     // H2R_ARENA_CHUNK_MB: physical chunk size of the arena's regions
    long pipe_sub_batch = 0;                     // H2R_PIPE_SUB_BATCH: elements per chain + record kernel pair inside a pipelined call (multiple of 256)
    long pipe_pace = -1;                         // H2R_PIPE_PACE=0|1: sub-batch i+1's chain kernel waits for sub-batch i-1's record kernel
    long pipe_step = -1;                         // H2R_PIPE_STEP=0: never issue a pipeline step as one launch (the two-queue form for every shape)
    long pipe_twoq_l16 = 0;                      // H2R_PIPE_TWOQ_L16=n: RSA-1024 takes the two-queue form for every call of up to n (-1: never; 0 = the measured rule)
    long pipe_form = -1;                         // H2R_PIPE_FORM=0|1: skip the queue probe; 1 = the two-queue form, 0 = the one-launch step
    long step_chain_x2_per_cu = 0;               // H2R_STEP_CHAIN_X2_PER_CU=n: n/2 chain workgroups per CU in a step launch (0 = the measured default)
    unsigned long pipe_cu_mask = 0;              // H2R_PIPE_CU_MASK=<hex word>: the record stream is created with this 32-bit CU mask repeated over the device (experiment)
    long pipe_cu_mask_words = 0;                 // H2R_PIPE_CU_MASK_WORDS=n: only the first n 32-bit words carry the mask, the rest are zero
    long verify_fold = -1;                       // H2R_VERIFY_FOLD=0|1: the verifier's witness inside the step launch's chain role (-1 = the measured default per shape)
    long exp_segments = -1;                      // H2R_EXP_SEGMENTS=n: segments a long exponent is walked in (0 / 1 = never; -1 = the default rule, exp_segment_count)
    long single_call_segments = -1;              // H2R_SINGLE_CALL_SEGMENTS=n: segments of a SHORT exponent in a single stream-ordered call of 513..1,536 RSA-2048 elements
    long rowprog_stage_rows = 0;                 // H2R_ROWPROG_STAGE_ROWS=64|128|256: rows (= threads) of a row-program workgroup (0 = the rule in launch_row_prog)
    long keep_const = -1;                        // H2R_KEEP_CONST=0: record launches into a trace arena's regions store the constant planes like any other
    long cells_nwv = 0;                          // H2R_CELLS_NWV=1|8: waves per cells_kernel workgroup of a Montgomery ctx (0 = the rule at ctx creation)
    long curve_ntt_form = 0;                     // H2R_CURVE_NTT_FORM=1: every butterfly of h2r_curve_ntt runs per-lane bit-by-bit double-and-add (the timing tool's baseline)
    Knobs() {
#ifdef H2R_DEV_KNOBS
        auto num = [](const char *name, long dflt) { const char *v = std::getenv(name); return v ? std::atol(v) : dflt; };
        chain_nw = (int)num("H2R_CHAIN_NW", 0); chain_deep = (int)num("H2R_CHAIN_DEEP", -1); chain_wave = num("H2R_CHAIN_WAVE", -1);
        trace_dyn_lds = num("H2R_TRACE_DYN_LDS", -1); trace_prio = num("H2R_TRACE_PRIO", -1);
        chain_prio = num("H2R_CHAIN_PRIO", -1); ablate = num("H2R_ABLATE", 0);
        const char *pe = std::getenv("H2R_PIPE_STREAM_PRIO");
        pipe_stream_prio = !pe ? -1 : (!std::strcmp(pe, "high") ? 1 : (!std::strcmp(pe, "low") ? -1 : 0));
        chain_timing = std::getenv("H2R_CHAIN_TIMING") != nullptr;
        { const char *g = std::getenv("H2R_PIPE_SERIALIZE"); pipe_serialize = g && g[0] == '1'; }
        { const char *m = std::getenv("H2R_PIPE_CU_MASK"); pipe_cu_mask = m ? std::strtoul(m, nullptr, 16) : 0; pipe_cu_mask_words = num("H2R_PIPE_CU_MASK_WORDS", 0); }
        verify_fold = num("H2R_VERIFY_FOLD", -1); exp_segments = num("H2R_EXP_SEGMENTS", -1); single_call_segments = num("H2R_SINGLE_CALL_SEGMENTS", -1);
        pipe_step = num("H2R_PIPE_STEP", -1); pipe_form = num("H2R_PIPE_FORM", -1); pipe_twoq_l16 = num("H2R_PIPE_TWOQ_L16", 0); step_chain_x2_per_cu = num("H2R_STEP_CHAIN_X2_PER_CU", 0);
        rowprog_stage_rows = num("H2R_ROWPROG_STAGE_ROWS", 0); cells_nwv = num("H2R_CELLS_NWV", 0);
        keep_const = num("H2R_KEEP_CONST", -1); curve_ntt_form = num("H2R_CURVE_NTT_FORM", 0);
        pipe_sub_batch = num("H2R_PIPE_SUB_BATCH", 0); arena_chunk_mb = num("H2R_ARENA_CHUNK_MB", 0); plain_overlap = num("H2R_PLAIN_OVERLAP", -1); pipe_pace = num("H2R_PIPE_PACE", -1);
#endif
    }
};
inline const Knobs &knobs() { static const Knobs k; return k; }   // one instance for the whole library (inline function, static local)

// Shapes with a compiled record kernel.  BigIntChip::new only asserts bits_len % limb_width == 0 (chip.rs:1175); here
// num_limbs must also be a multiple of 4 (64-bit limbs, up to 4096 bits: RSA-1024/1536/2048/3072/4096 ...) or of 8
// (32-bit limbs, up to 4096 bits), so that every accumulator row is a whole number of 64-byte store segments.
constexpr u32 kLStep64 = 4, kLMax64 = 64, kLStep32 = 8, kLMax32 = 128;
inline bool shape_supported(u32 w, u32 L) {
    if (w == 64) return L >= kLStep64 && L <= kLMax64 && L % kLStep64 == 0;
    if (w == 32) return L >= kLStep32 && L <= kLMax32 && L % kLStep32 == 0;
    return false;
}

// The shapes with a step build: (limb width, limbs) -> (chain digits K, waves NW).  A step's workgroup is the chain role's.
struct StepShape { u32 w, L, K, NW; };
constexpr StepShape kStepShapes[] = {{64, 32, 64, 4}, {64, 16, 32, 4}, {32, 128, 128, 8}, {64, 64, 128, 8}, {64, 48, 96, 6}};
inline const StepShape *step_shape_of(u32 w, u32 L, u32 K) {
    for (const StepShape &s : kStepShapes) if (w == s.w && L == s.L && K == s.K) return &s;
    return nullptr;
}

// h2r_tu_trace.hip.  ea/eb (nullable): start/stop events stamped by the dispatch itself.
hipError_t launch_trace_shape(u32 w, u32 L, u32 lds_per_cu, const TraceArgs &ta, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_chain.hip.  co_running: the call's record kernel of the PREVIOUS batch runs next to this chain kernel (pipeline mode)
hipError_t launch_chain_shape(u32 num_cus, const ChainArgs &ca, bool co_running, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_chain_shape_keyed(u32 num_cus, const ChainArgs &ca, bool co_running, hipStream_t st, hipEvent_t ea, hipEvent_t eb);   // h2r_tu_chain_keyed.hip
// The key table of keyed moduli: K of the chain build for `kreal` digits (what the entries are computed for), and the kernel that fills
// the table's two planes (raw digits, raw_stride per entry; chain_pre_words(K) words of Barrett constants per entry) plus the sentinel entry.
u32 chain_digits(u32 kreal);
hipError_t launch_key_table_shape(const u32 *n_keys, u32 kreal, u64 num_keys, u32 *raw, u32 raw_stride, u32 *pre, u8 *key_status, hipStream_t st);
// h2r_tu_step.hip.  One step: the records described by `ta` (an earlier sub-batch) and the chains described by `ca`, one launch on `st`.
hipError_t launch_step_shape(const StepShape &s, u32 num_cus, const ChainArgs &ca, const TraceArgs &ta, const AuxArgs *aa, const AuxArgs *va,
                             const Sha256Args *sha, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_step_shape_keyed(const StepShape &s, u32 num_cus, const ChainArgs &ca, const TraceArgs &ta, const AuxArgs *aa, const AuxArgs *va,
                                   const Sha256Args *sha, hipStream_t st, hipEvent_t ea, hipEvent_t eb);   // h2r_tu_step_keyed.hip
u32 step_shared_bytes_shape(const StepShape &s);
// h2r_tu_cells.hip.  `lds` = the dynamic LDS request (residency rule applied by the caller); nwv = waves per workgroup (Montgomery, long shapes).
hipError_t launch_cells_shape(u32 w, bool mont, u32 nwv, u32 lds, const CellsArgs &ca, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_lookup_product.hip (argument structs: h2r_lookup_product.hpp).  The grand product's three phases (h2r_grand_product.hpp): 0 = the tiles'
// products, 1 = the carry-ins per column, 2 = the scans that write Z.
struct LookupInputArgs;
struct LookupProductArgs;
hipError_t launch_lookup_input(const LookupInputArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_lookup_product(u32 phase, const LookupProductArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_permutation_product.hip (argument struct: h2r_permutation_product.hpp).  The same three phases of the same core: per tile of a set, per
// element (one wave walks its sets), per tile of a set.
struct PermProductArgs;
hipError_t launch_perm_product(u32 phase, const PermProductArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_ntt.hip (argument structs: h2r_ntt.hpp).  The twiddle tables of one call, then one pass (a.pass) over num_cols x num_elems columns.
struct NttSetupArgs;
struct NttArgs;
hipError_t launch_ntt_setup(const NttSetupArgs &a, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_ntt_pass(const NttArgs &a, u32 num_cols, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_quotient.hip (argument struct: h2r_quotient.hpp).  The tiles [a.tile0, a.tile0 + num_tiles) of num_elems circuits.
struct QuotientArgs;
hipError_t launch_quotient(const QuotientArgs &a, u32 num_tiles, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_open.hip (argument structs: h2r_open.hpp).  phase 0 = the tiles' sums, 1 = the carries and the evaluations, 2 = the scans that write W;
// the circuits [a.elem0, a.elem0 + num_elems).  The fold: the tiles [a.tile0, a.tile0 + num_tiles) of num_elems circuits.
struct OpenArgs;
struct FoldArgs;
hipError_t launch_open(u32 phase, const OpenArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_fold(const FoldArgs &a, u32 num_tiles, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_msm.hip (argument struct: h2r_msm.hpp).  phase 0 = the buckets of every (slice, window, column), 1 = the fold per column; the circuits
// [a.elem0, a.elem0 + num_elems).
struct MsmArgs;
hipError_t launch_msm(u32 phase, const MsmArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_curve_ntt.hip (argument struct: h2r_curve_ntt.hpp).  phase 0 = the twiddle table, 1 = the load, 2 = stage a.stage, 3 = the store; the
// workgroups [a.block0, a.block0 + num_blocks) of 256 twiddles / points / butterflies / points.
struct CurveNttArgs;
hipError_t launch_curve_ntt(u32 phase, const CurveNttArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_transcript.hip (argument struct: h2r_transcript.hpp).  One round of the workgroups [a.block0, a.block0 + num_blocks) of 64 circuits.
struct TranscriptArgs;
hipError_t launch_transcript(const TranscriptArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_random.hip (argument struct: h2r_random.hpp).  The row tiles [a.tile0, a.tile0 + num_tiles) of num_cols columns of the circuits
// [a.elem0, a.elem0 + num_elems).
struct RandomArgs;
hipError_t launch_random(const RandomArgs &a, u32 num_tiles, u32 num_cols, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_verify.hip (argument structs: h2r_verify.hpp).  Decode: pass a.pass over the workgroups [a.block0, a.block0 + num_blocks) of 64 circuits x
// a.num_items items (grid.y).  Scalars: the workgroups [a.block0, a.block0 + num_blocks) of 64 circuits.  Terms: the circuits [a.elem0, a.elem0 + num_elems).
struct DecodeArgs;
struct VerifyScalarsArgs;
struct MsmTermsArgs;
hipError_t launch_proof_decode(const DecodeArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_verify_scalars(const VerifyScalarsArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_msm_terms(const MsmTermsArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_pairing.hip (argument struct: h2r_pairing.hpp).  The workgroups [a.block0, a.block0 + num_blocks) of 8 circuits.
struct PairingArgs;
hipError_t launch_pairing(const PairingArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_keygen.hip (argument structs: h2r_keygen.hpp).  The fixed columns: one launch over every (row, column).  Sigma: phase = KG_PHASE_*,
// the grid follows from the arguments (pairs, tiles of ids, tiles of sorted entries).
struct KeygenFixedArgs;
struct KeygenSigmaArgs;
hipError_t launch_keygen_fixed(const KeygenFixedArgs &a, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_keygen_sigma(u32 phase, const KeygenSigmaArgs &a, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_setup.hip (argument structs: h2r_setup.hpp).  The table: the windows [a.block0, a.block0 + num_blocks), one workgroup each.  The
// multiplication and the scalars: the workgroups [a.block0, a.block0 + num_blocks) of 256 scalars.
struct FixedBaseTableArgs;
struct FixedBaseMulArgs;
struct SetupScalarsArgs;
hipError_t launch_fixed_base_table(const FixedBaseTableArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_fixed_base_mul(const FixedBaseMulArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_setup_scalars(const SetupScalarsArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
// h2r_tu_witness.hip (argument structs: h2r_kernels.hpp, h2r_muled.hpp).  w = the limb width (64 | 32).  The aux kernel is the keyed build when
// aa.key_idx is set; `lds` / `stage` = the dynamic LDS request.
struct RefreshArgs;
struct EqMuledArgs;
struct PadArgs;
struct ArenaConstPlanes { u64 off[7]; u32 bytes[7]; };   // the constant planes of a record: offsets in the record, bytes (whole words)
hipError_t launch_aux_shape(u32 w, u32 lds, const AuxArgs &aa, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_fresh_shape(u32 w, const FreshArgs &fa, hipStream_t st);
hipError_t launch_sha256(const Sha256Args &sa, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_check_shape(u32 w, const CheckArgs &ca, hipStream_t st);
hipError_t launch_link_shape(u32 w, const LinkArgs &la, u64 batch, hipStream_t st);
hipError_t launch_decompose(const DecompArgs &da, u32 blocks, hipStream_t st);
hipError_t launch_key_expand(const u32 *raw, u32 raw_stride, u32 num_keys, const u32 *key_idx, u64 batch, u32 kreal, u32 *n_out, hipStream_t st);
hipError_t launch_refresh(const RefreshArgs &ra, u32 stage, hipStream_t st);
hipError_t launch_is_equal_muled(const EqMuledArgs &ea, u32 stage, hipStream_t st);
hipError_t launch_pad_limbs(const PadArgs &pa, hipStream_t st);
hipError_t launch_arena_fill(u8 *p, u64 bytes, hipStream_t st, hipEvent_t ea, hipEvent_t eb);   // one workgroup per 64 KB
hipError_t launch_arena_restore(u32 blocks, u8 *base, u64 elem_stride, u64 off_records, u64 record_stride, u32 T, u64 n_records, const u8 *cr,
                                const ArenaConstPlanes &pl, hipStream_t st);
hipError_t launch_queue_probe(unsigned long long ticks, unsigned long long *stamp, hipStream_t st);
// h2r_tu_advice.hip (argument structs: h2r_kernels.hpp, h2r_varrows.hpp, h2r_rowprog.hpp, h2r_copymap.hpp, h2r_check.hpp).  sr = rows (= threads)
// of a row-program workgroup (64 | 128 | 256), nt = threads of an inverse-witness workgroup (64 | 256); `blocks` = the grid.
struct VarRowsArgs;
struct RowProgArgs;
struct LayoutArgs;
struct AdviceCheckArgs;
struct AdviceHistArgs;
hipError_t launch_advice_shape(u32 w, const AdviceArgs &aa, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_emit_shape(u32 w, const EmitArgs &a, u32 blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_var_rows_shape(u32 w, const VarRowsArgs &va, u32 blocks, hipStream_t st);
hipError_t launch_rowprog_shape(u32 w, u32 sr, const RowProgArgs &ra, u32 blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb);
hipError_t launch_rowprog_inv_shape(u32 w, u32 nt, const RowProgArgs &ra, u32 blocks, hipStream_t st);
hipError_t launch_advice_layout(const LayoutArgs &la, u32 blocks, hipStream_t st);
hipError_t launch_advice_check_rows(const AdviceCheckArgs &ca, u32 blocks, hipStream_t st);
hipError_t launch_advice_check_copies(const AdviceCheckArgs &ca, u32 blocks, hipStream_t st);
hipError_t launch_advice_hist(const AdviceHistArgs &ha, u32 blocks, hipStream_t st);
// h2r_tu_lookup.hip (argument structs: h2r_kernels.hpp, h2r_lookup.hpp).  One workgroup per element (hist, perm, the three histograms), per
// element and argument (set-up), per chunk of a.rows_per_block rows, argument and element (fill).  perm: `staged` = 16-bit cell ids in LDS.
struct LookupHistArgs;
struct LookupValuesArgs;
struct LookupFreshArgs;
struct LookupSetupArgs;
struct LookupFillArgs;
hipError_t launch_hist(const HistArgs &ha, hipStream_t st);
hipError_t launch_perm(bool staged, u32 lds, const PermArgs &pa, hipStream_t st);
hipError_t launch_lookup_hist_records(const LookupHistArgs &a, hipStream_t st);
hipError_t launch_lookup_hist_values(const LookupValuesArgs &a, hipStream_t st);
hipError_t launch_lookup_hist_fresh(const LookupFreshArgs &a, hipStream_t st);
hipError_t launch_lookup_setup(const LookupSetupArgs &a, hipStream_t st);
hipError_t launch_lookup_fill(const LookupFillArgs &a, hipStream_t st, hipEvent_t ea, hipEvent_t eb);

}  // namespace h2r
