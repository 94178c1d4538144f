"""The prover stages on the device: halo2's lookup and permutation arguments, the evaluation domain (transforms, quotient, openings) and
the commitment key, the Fiat-Shamir transcript that joins them, the generator of the blinding values, create_proof, which runs them in halo2's order, verify_proof and verify, the verifier to its verdict, keygen, and setup, the KZG parameters of a known tau.  None of them has a counterpart in the reference's `big_integer`
module; `big_integer` re-exports the five classes.
All arithmetic happens in libh2r.so; every method marshals its arguments with `_marshal` and makes the call.
A chip is whatever has `_ctx`, `_stream()`, `device` and `montgomery` (big_integer.BigIntChip)."""
import ctypes
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from ._marshal import challenges, column_group, from_words, hold, image_stride, is_columns, kinds_tensor, outputs, ptr, ref, set_words, words, workspace


class LookupArgument:
    """halo2's lookup argument for the range checks (h2r_lookup_*): RangeChip's (tag, value) table, the per-argument
    multiplicities of a batch of circuits and the permuted columns A' / S' for per-circuit challenges theta.
    Third-party behaviour restated in DESIGN.md section 2c; five arguments: composition_a..d, overflow_a."""

    ARGS = 5

    def __init__(self, chip: "BigIntChip", rsa_chip: bool = True, bit_lens: Optional[Sequence[int]] = None,
                 tags: Optional[Sequence[int]] = None):
        self.chip = chip
        self.cfg = _lib.H2RLookupConfig()
        if bit_lens is None:
            check(lib().h2r_lookup_config_default(chip._ctx, 1 if rsa_chip else 0, ctypes.byref(self.cfg)), "h2r_lookup_config_default")
        else:
            n = len(bit_lens)
            check(lib().h2r_lookup_config_custom((ctypes.c_uint32 * n)(*bit_lens), (ctypes.c_uint32 * n)(*tags), n, ctypes.byref(self.cfg)),
                  "h2r_lookup_config_custom")
        self.n_rows = int(self.cfg.n_rows)

    def table_image(self):
        """[(tag, value)] as load_table writes them (canonical field elements; small integers)."""
        t = np.zeros((self.n_rows, 4), dtype=np.uint64)
        v = np.zeros((self.n_rows, 4), dtype=np.uint64)
        check(lib().h2r_lookup_table_image(self.chip._ctx, ctypes.byref(self.cfg), t.ctypes.data, v.ctypes.data), "h2r_lookup_table_image")
        return [(int(a[0]), int(b[0])) for a, b in zip(t, v)]

    def new_hist(self, batch: int) -> torch.Tensor:
        return torch.zeros((batch, self.ARGS, self.n_rows), dtype=torch.int32, device="cuda:%d" % self.chip.device)

    def hist_records(self, trace: "Trace", hist: torch.Tensor, status: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Adds the lookups of every mul_mod record of every element (q / r limbs, range-assigned carries)."""
        off = trace.pow_layout.off_records if trace.pow_layout is not None else 0
        check(lib().h2r_lookup_hist_records(self.chip._ctx, ctypes.byref(self.cfg), trace.buf.data_ptr(), off, trace.elem_stride, trace.batch,
                                            trace.num_mul_mods, ptr(status), hist.data_ptr(), self.chip._stream()), "h2r_lookup_hist_records")
        return hist

    def hist_values(self, values: torch.Tensor, bit_len: int, sublimb_bits: int, hist: torch.Tensor) -> torch.Tensor:
        """Adds RangeChip::assign(v, sublimb_bits, bit_len) of values[elem][:] (int32 / int64 elements)."""
        assert values.dim() == 2 and values.is_contiguous()
        check(lib().h2r_lookup_hist_values(self.chip._ctx, ctypes.byref(self.cfg), values.data_ptr(), values.element_size(), values.shape[1],
                                           values.shape[0], bit_len, sublimb_bits, hist.data_ptr(), self.chip._stream()), "h2r_lookup_hist_values")
        return hist

    def hist_fresh_op(self, op_name: str, trace_buf: torch.Tensor, elem_stride: int, batch: int, hist: torch.Tensor, first_off: int = 0):
        """Adds the range assigns inside a Fresh-op witness (e.g. "is_in_field": the assert_in_field witness of modpow_public_key)."""
        check(lib().h2r_lookup_hist_fresh_op(self.chip._ctx, ctypes.byref(self.cfg), _lib.FRESH_OPS.index(op_name), trace_buf.data_ptr(), first_off,
                                             elem_stride, batch, hist.data_ptr(), self.chip._stream()), "h2r_lookup_hist_fresh_op")
        return hist

    def hist_advice(self, kinds, image: torch.Tensor, batch: int, hist: torch.Tensor, status: Optional[torch.Tensor] = None, layout=None) -> torch.Tensor:
        """The multiplicities of an advice image (h2r_lookup_hist_advice): what hist_verify / hist_records / hist_fresh_op count from a trace,
        for a witness without records.  kinds: uint8 row kinds (numpy or device tensor)."""
        kd = kinds_tensor(kinds, image.device)
        check(lib().h2r_lookup_hist_advice(self.chip._ctx, ctypes.byref(self.cfg), ref(layout), kd.data_ptr(), kd.numel(), image.data_ptr(),
                                           image_stride(image, batch), batch, ptr(status), hist.data_ptr(), self.chip._stream()), "h2r_lookup_hist_advice")
        hold(self, "hist_advice", kd)
        return hist

    def hist_verify(self, res, hist: torch.Tensor) -> torch.Tensor:
        """Every lookup inside the witness of a verify_pkcs1v15_signature batch (rsa.VerifyResult): assert_in_field's range assigns,
        the records' limbs and carries, the encoded-message check's two 4-bit range assigns (h2r_lookup_hist_verify)."""
        check(lib().h2r_lookup_hist_verify(self.chip._ctx, ctypes.byref(self.cfg), ctypes.byref(res.layout), res.trace.data_ptr(),
                                           res.is_valid.numel(), res.status.data_ptr(), hist.data_ptr(), self.chip._stream()), "h2r_lookup_hist_verify")
        return hist

    def permuted_columns(self, hist: torch.Tensor, thetas: Sequence[int], usable_rows: int, arg_mask: int = 31, out=None):
        """(A', S', status): uint8 [batch, 5, usable_rows, 32] each -- canonical little-endian field elements."""
        batch, dev = hist.shape[0], hist.device
        th_dev = challenges(thetas, dev, batch)
        cols = (torch.empty, torch.uint8, (batch, self.ARGS, usable_rows, 32))
        a_perm, s_perm = outputs(out, dev, cols, cols)
        status = torch.zeros(batch, dtype=torch.uint8, device=dev)
        ws = workspace(lib().h2r_lookup_workspace_bytes(ctypes.byref(self.cfg), batch), dev, floor=0)
        check(lib().h2r_lookup_permuted_columns(self.chip._ctx, ctypes.byref(self.cfg), hist.data_ptr(), th_dev.data_ptr(), batch, usable_rows,
                                                arg_mask, a_perm.data_ptr(), s_perm.data_ptr(), self.ARGS * usable_rows * 32, status.data_ptr(),
                                                ws.data_ptr(), self.chip._stream()), "h2r_lookup_permuted_columns")
        hold(self, "permuted_columns", th_dev, ws)
        return a_perm, s_perm, status

    def input_columns(self, kinds, image: torch.Tensor, batch: int, thetas: Sequence[int], usable_rows: int, status: Optional[torch.Tensor] = None,
                      layout=None, first_row: int = 0, arg_mask: int = 31, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A: uint8 [batch, 5, usable_rows, 32], the compressed lookup inputs of an advice image in ORIGINAL row order (h2r_lookup_input_columns);
        the image's rows sit at first_row, every other usable row is 0.  thetas and A in the ctx's representation."""
        kd = kinds_tensor(kinds, image.device)
        th_dev = challenges(thetas, image.device, batch)
        a_in = outputs(out, image.device, (torch.empty, torch.uint8, (batch, self.ARGS, usable_rows, 32)))
        check(lib().h2r_lookup_input_columns(self.chip._ctx, ctypes.byref(self.cfg), ref(layout), kd.data_ptr(), kd.numel(), image.data_ptr(),
                                             image_stride(image, batch), batch, ptr(status), th_dev.data_ptr(), usable_rows, first_row, arg_mask,
                                             a_in.data_ptr(), self.ARGS * usable_rows * 32, self.chip._stream()), "h2r_lookup_input_columns")
        hold(self, "input_columns", kd, th_dev)
        return a_in

    def product_columns(self, a_in: torch.Tensor, a_perm: torch.Tensor, s_perm: torch.Tensor, thetas: Sequence[int], betas: Sequence[int],
                        gammas: Sequence[int], usable_rows: int, arg_mask: int = 31, out=None):
        """(Z, status): Z uint8 [batch, 5, usable_rows + 1, 32], halo2's lookup grand product (h2r_lookup_product_columns) in the ctx's
        representation; status H2R_E_ASSERTION where a denominator is zero or Z[usable_rows] != 1, H2R_E_SHAPE where a challenge is not canonical.
        out: (z, status) to write into (a status byte that is nonzero on entry skips the circuit; the call never clears it)."""
        batch, dev = a_in.shape[0], a_in.device
        ch = [challenges(v, dev, batch) for v in (thetas, betas, gammas)]
        z, status = outputs(out, dev, (torch.empty, torch.uint8, (batch, self.ARGS, usable_rows + 1, 32)), status=batch)
        ws = workspace(lib().h2r_lookup_product_workspace_bytes(usable_rows, batch), dev, floor=0)
        col = (usable_rows + 1) * 32
        check(lib().h2r_lookup_product_columns(self.chip._ctx, ctypes.byref(self.cfg), a_in.data_ptr(), a_perm.data_ptr(), s_perm.data_ptr(),
                                               self.ARGS * usable_rows * 32, ch[0].data_ptr(), ch[1].data_ptr(), ch[2].data_ptr(), batch, usable_rows,
                                               arg_mask, z.data_ptr(), self.ARGS * col, col, status.data_ptr(), ws.data_ptr(), self.chip._stream()),
              "h2r_lookup_product_columns")
        hold(self, "product_columns", ch, ws)
        return z, status


def _permutation_columns(cfg, column_src):
    """column_src (per permutation column 0..4 = physical advice column, 5 + j = extra column j) and what follows from it, into a config."""
    cfg.num_columns = len(column_src)
    cfg.n_extra = max([int(s) - 4 for s in column_src if int(s) >= 5] + [0])
    for c, s in enumerate(column_src):
        cfg.column_src[c] = int(s)


class PermutationArgument:
    """halo2's permutation (copy-constraint) argument: the grand-product columns Z of permutation::prover::commit for per-circuit
    challenges beta, gamma (h2r_permutation_product_columns).  Third-party behaviour restated in DESIGN.md section 2e.  The sigma columns
    belong to the proving key and are the caller's.  column_src: per permutation column 0..4 = physical advice column, 5 + j = extra
    column j; chunk_len = cs_degree - 2; delta, omega: integers in the chip's representation."""

    def __init__(self, chip: "BigIntChip", column_src: Sequence[int], chunk_len: int, delta: int, omega: int):
        self.chip = chip
        self.cfg = cfg = _lib.H2RPermutationConfig(struct_size=ctypes.sizeof(_lib.H2RPermutationConfig), chunk_len=chunk_len)
        if len(column_src) > _lib.H2R_PERM_MAX_COLUMNS:
            check(_lib.H2R_E_SHAPE, "PermutationArgument")
        _permutation_columns(cfg, column_src)
        set_words(cfg.delta, delta)
        set_words(cfg.omega, omega)
        self.sets = int(lib().h2r_permutation_sets(ctypes.byref(cfg)))
        if self.sets == 0:
            check(_lib.H2R_E_SHAPE, "h2r_permutation_sets")

    def product_columns(self, image: torch.Tensor, batch: int, rows: int, sigma: torch.Tensor, betas: Sequence[int], gammas: Sequence[int],
                        usable_rows: int, first_row: int = 0, extra: Optional[torch.Tensor] = None, out=None):
        """(Z, status): Z uint8 [batch, S, usable_rows + 1, 32] in the chip's representation; status H2R_E_ASSERTION where a set's
        denominators multiply to zero or the last Z does not end at 1, H2R_E_SHAPE where a challenge is not canonical.
        image: the advice image of `rows` rows per circuit, at first_row of the usable rows; sigma: uint8 [m, >= usable_rows, 32] shared by
        every circuit; extra: uint8 [batch, n_extra, >= usable_rows, 32]; betas / gammas: integers in the chip's representation.
        out: (z, status) to write into (a status byte that is nonzero on entry skips the circuit; the call never clears it)."""
        dev = image.device
        ch = [challenges(v, dev, batch) for v in (betas, gammas)]
        z, status = outputs(out, dev, (torch.empty, torch.uint8, (batch, self.sets, usable_rows + 1, 32)), status=batch)
        assert is_columns(sigma, dims=(3,)) and sigma.shape[0] == self.cfg.num_columns
        assert extra is None or is_columns(extra, dims=(4,))
        ws = workspace(lib().h2r_permutation_product_workspace_bytes(ctypes.byref(self.cfg), usable_rows, batch), dev, floor=0)
        check(lib().h2r_permutation_product_columns(self.chip._ctx, ctypes.byref(self.cfg), image.data_ptr(), image_stride(image, batch), rows,
                                                    first_row, batch, *(column_group(extra, True) if extra is not None else (None, 0, 0)), sigma.data_ptr(), sigma.stride(0),
                                                    ch[0].data_ptr(), ch[1].data_ptr(), usable_rows, z.data_ptr(), z.stride(0), z.stride(1),
                                                    status.data_ptr(), ws.data_ptr(), self.chip._stream()), "h2r_permutation_product_columns")
        hold(self, "product_columns", ch, ws, sigma, extra, image)
        return z, status


class EvaluationDomain:
    """halo2's poly::domain::EvaluationDomain on the device (h2r_ntt_columns; third-party behaviour restated in DESIGN.md section 2f):
    the transforms between Lagrange, coefficient and extended (coset) form of columns of 2^k / 2^extended_k field elements.
    omega_ext: a primitive 2^extended_k-th root of unity, zeta: the extended domain's coset shift (both integers in the chip's
    representation); omega at k is omega_ext^(2^(extended_k - k)).  Columns are uint8 tensors [..., rows, 32] (up to two leading
    dimensions: [batch, columns, rows, 32]) whose last two dimensions are contiguous, in the chip's representation."""

    def __init__(self, chip: "BigIntChip", k: int, extended_k: int, omega_ext: int, zeta: int):
        if not 1 <= k <= extended_k:
            check(_lib.H2R_E_SHAPE, "EvaluationDomain")
        self.chip, self.k, self.extended_k, self.omega_ext, self.zeta = chip, int(k), int(extended_k), int(omega_ext), int(zeta)
        self.one = self._field(_lib.FIELD_TO_MONTGOMERY, 1) if chip.montgomery else 1
        self.omega = self.omega_at(self.k)

    def _field(self, op: int, a: int, b: int = 0) -> int:
        wa, wb, out = ((ctypes.c_uint64 * 4)(*words(v)) for v in (a, b, 0))
        check(lib().h2r_field_eval(self.chip._ctx, op, wa, wb, out), "h2r_field_eval")
        return from_words(out)

    def omega_at(self, log_n: int) -> int:
        """omega_ext^(2^(extended_k - log_n)): the generator of the 2^log_n domain, in the chip's representation."""
        if not 0 < log_n <= self.extended_k:
            check(_lib.H2R_E_SHAPE, "EvaluationDomain.omega_at")
        w = self._field(_lib.FIELD_FROM_MONTGOMERY, self.omega_ext) if self.chip.montgomery else self.omega_ext
        for _ in range(self.extended_k - log_n):
            w = self._field(_lib.FIELD_MUL, w, w)
        return self._field(_lib.FIELD_TO_MONTGOMERY, w) if self.chip.montgomery else w

    def ntt(self, cols: torch.Tensor, log_n_out: int, inverse: bool = False, shift: Optional[int] = None, out: Optional[torch.Tensor] = None):
        """The raw transform: forward out[j] = sum_i cols[i] * (shift * omega^j)^i onto 2^log_n_out points (the input zero-padded), or the
        inverse of it (log_n_out = the input's size).  shift: an integer in the chip's representation (None: 1, no coset).
        out: a tensor of the input's leading shape with 2^log_n_out rows to write into (it must not overlap the input)."""
        rows = cols.shape[-2]
        if not is_columns(cols, dims=(2, 3, 4), strides=False) or rows & (rows - 1) or rows == 0:
            check(_lib.H2R_E_SHAPE, "EvaluationDomain.ntt")
        assert is_columns(cols)
        cfg = _lib.H2RNttConfig(struct_size=ctypes.sizeof(_lib.H2RNttConfig), log_n_in=rows.bit_length() - 1, log_n_out=log_n_out,
                                flags=_lib.H2R_NTT_INVERSE if inverse else 0)
        set_words(cfg.omega, self.omega_at(log_n_out))
        set_words(cfg.shift, self.one if shift is None else shift)
        lead = tuple(cols.shape[:-2])
        out = outputs(out, cols.device, (torch.empty, torch.uint8, lead + (1 << log_n_out, 32)))
        assert tuple(out.shape[:-2]) == lead and is_columns(out, rows=1 << log_n_out)
        (_, ies, ics), (_, oes, ocs) = column_group(cols, len(lead) == 2), column_group(out, len(lead) == 2)
        batch, ncols = ((1, 1) + lead)[-2:]
        if len(lead) < 2:   # one element: its stride is the reach of its columns
            ies, oes = max(rows * 32, ncols * ics), max(32 << log_n_out, ncols * ocs)
        ws = workspace(lib().h2r_ntt_workspace_bytes(ctypes.byref(cfg)), cols.device)
        check(lib().h2r_ntt_columns(self.chip._ctx, ctypes.byref(cfg), cols.data_ptr(), ies, ics, out.data_ptr(), oes, ocs, ncols, batch,
                                    ws.data_ptr(), self.chip._stream()), "h2r_ntt_columns")
        hold(self, "ntt", ws, cols, out)
        return out

    def lagrange_to_coeff(self, cols: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """2^k evaluations over the domain -> the 2^k coefficients."""
        return self.ntt(cols, self.k, inverse=True, out=out)

    def coeff_to_extended(self, cols: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """2^k coefficients -> the 2^extended_k evaluations over the coset zeta * <omega_ext>."""
        return self.ntt(cols, self.extended_k, shift=self.zeta, out=out)

    def extended_to_coeff(self, cols: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """2^extended_k evaluations over the coset -> the 2^extended_k coefficients (truncation stays the caller's)."""
        return self.ntt(cols, self.extended_k, inverse=True, shift=self.zeta, out=out)

    def lagrange_key(self, key: "CommitKey") -> "CommitKey":
        """The Lagrange-basis key of this domain over the first 2^k bases of `key` (halo2's g_lagrange from g): key.transform(omega, k)."""
        return key.transform(self.omega, self.k)

    def vanishing_columns(self, blinding_factors: int) -> torch.Tensor:
        """uint8 [3, 2^extended_k, 32]: l0, l_last and l_active = 1 - l_last - l_blind of the 2^k domain with `blinding_factors` blinding
        rows, in extended form (lagrange_to_coeff, then coeff_to_extended) -- the `l` columns of quotient()."""
        n = 1 << self.k
        u = n - blinding_factors - 1
        if u < 1:
            check(_lib.H2R_E_SHAPE, "EvaluationDomain.vanishing_columns")
        host = np.zeros((3, n, 32), dtype=np.uint8)
        one = np.frombuffer(int(self.one).to_bytes(32, "little"), dtype=np.uint8)
        host[0, 0] = one
        host[1, u] = one
        host[2, :u] = one
        lag = torch.from_numpy(host).to("cuda:%d" % self.chip.device)
        return self.coeff_to_extended(self.lagrange_to_coeff(lag))

    def quotient(self, blinding_factors: int, delta: int, gate_fixed: Sequence[int], column_src: Sequence[int], chunk_len: int, advice: torch.Tensor,
                 perm_z: torch.Tensor, fixed: torch.Tensor, sigma: torch.Tensor, l: torch.Tensor, thetas: Sequence[int], betas: Sequence[int],
                 gammas: Sequence[int], ys: Sequence[int], extra: Optional[torch.Tensor] = None, lookup_mask: int = 0,
                 lookup_advice: Sequence[int] = (0, 1, 2, 3, 0), lookup_tag: Sequence[int] = (0,) * 5, lookup_enable: Sequence[int] = (0,) * 5,
                 table_tag: int = 0, table_value: int = 0, lookup_a_perm: Optional[torch.Tensor] = None, lookup_s_perm: Optional[torch.Tensor] = None,
                 lookup_z: Optional[torch.Tensor] = None, out=None):
        """(h, status): the vanishing argument's quotient on the extended domain (h2r_quotient_columns; halo2's evaluate_h for this circuit's
        constraint system, restated in DESIGN.md section 2g).  h: uint8 [batch, 2^extended_k, 32] in the chip's representation; status
        H2R_E_SHAPE where a challenge is not canonical (that circuit's h is left untouched).
        Every column is in extended form, uint8 with N = 2^extended_k rows whose last two dimensions are contiguous.  Per circuit
        [batch, columns, N, 32]: advice (5, physical), extra (n_extra), perm_z (S), lookup_a_perm / lookup_s_perm / lookup_z (column k =
        argument k, up to the highest bit of lookup_mask).  The proving key's [columns, N, 32]: fixed, sigma (one per permutation column), l
        (vanishing_columns()).  gate_fixed: the indices of sa, sb, sc, sd, se, s_mul_ab, s_mul_cd, se_next, s_const among the fixed columns;
        column_src / chunk_len as PermutationArgument; lookup_advice / lookup_tag / lookup_enable / table_tag / table_value: per argument
        the physical advice column and the fixed columns of its input expression theta * tag + enable * advice, and of the table's.
        delta and the challenges: integers in the chip's representation.  out: (h, status) to write into (h must overlap no input; a
        status byte that is nonzero on entry skips the circuit; the call never clears it)."""
        N = 1 << self.extended_k
        batch, dev = advice.shape[0], advice.device
        cfg = _lib.H2RQuotientConfig(struct_size=ctypes.sizeof(_lib.H2RQuotientConfig), log_n=self.k, log_ext=self.extended_k, blinding_factors=blinding_factors)
        set_words(cfg.omega_ext, self.omega_ext)
        set_words(cfg.zeta, self.zeta)
        set_words(cfg.delta, delta)
        if len(column_src) > _lib.H2R_PERM_MAX_COLUMNS or len(gate_fixed) != 9 or any(len(x) != _lib.H2R_LOOKUP_ARGS for x in (lookup_advice, lookup_tag, lookup_enable)):
            check(_lib.H2R_E_SHAPE, "EvaluationDomain.quotient")
        cfg.num_fixed, cfg.chunk_len, cfg.lookup_mask = fixed.shape[0], chunk_len, lookup_mask
        _permutation_columns(cfg, column_src)
        for i, v in enumerate(gate_fixed):
            cfg.gate_fixed[i] = int(v)
        for k in range(_lib.H2R_LOOKUP_ARGS):
            cfg.lookup_advice[k], cfg.lookup_tag[k], cfg.lookup_enable[k] = int(lookup_advice[k]), int(lookup_tag[k]), int(lookup_enable[k])
        cfg.table_tag, cfg.table_value = int(table_tag), int(table_value)
        inp = _lib.H2RQuotientInputs()
        per_circuit = {"advice": advice, "extra": extra, "perm_z": perm_z, "lookup_a_perm": lookup_a_perm, "lookup_s_perm": lookup_s_perm,
                       "lookup_z": lookup_z}
        for name, t in list(per_circuit.items()) + [("fixed", fixed), ("sigma", sigma), ("l", l)]:
            if t is not None:
                pc = name in per_circuit
                assert is_columns(t, rows=N, dims=(4 if pc else 3,), batch=batch if pc else None), name
                g = getattr(inp, name)
                g.base, g.elem_stride, g.col_stride = column_group(t, pc)
        ch = [challenges(v, dev, batch) for v in (thetas, betas, gammas, ys)]
        inp.theta, inp.beta, inp.gamma, inp.y = (c.data_ptr() for c in ch)
        h, status = outputs(out, dev, (torch.empty, torch.uint8, (batch, N, 32)), status=batch)
        assert is_columns(h, rows=N, dims=(3,))
        check(lib().h2r_quotient_columns(self.chip._ctx, ctypes.byref(cfg), ctypes.byref(inp), batch, h.data_ptr(), h.stride(0), ptr(status),
                                         self.chip._stream()), "h2r_quotient_columns")
        hold(self, "quotient", ch, advice, extra, perm_z, lookup_a_perm, lookup_s_perm, lookup_z, fixed, sigma, l, h, status)
        return h, status

    def fold(self, cols: torch.Tensor, scalars: Sequence[int], out=None):
        """(folded, status): folded[e][i] = sum_c scalars[e]^c * cols[e][c][i] (h2r_fold_columns), uint8 [batch, n, 32].
        cols: uint8 [batch, C, n, 32] in coefficient form, last two dimensions contiguous; with the 2^extended_k coefficients of h viewed
        as [batch, 2^(extended_k - k), 2^k, 32] and scalars = x^n it is the folded h of vanishing::prover::evaluate.  scalars: integers in
        the chip's representation; status H2R_E_SHAPE where one is not canonical (that circuit is left untouched).  out: (folded, status)
        to write into (it must overlap no input; a status byte that is nonzero on entry skips the circuit; the call never clears it)."""
        if not is_columns(cols, dims=(4,), strides=False):
            check(_lib.H2R_E_SHAPE, "EvaluationDomain.fold")
        assert is_columns(cols)
        batch, C, n = cols.shape[:3]
        s = challenges(scalars, cols.device, batch)
        folded, status = outputs(out, cols.device, (torch.empty, torch.uint8, (batch, n, 32)), status=batch)
        assert is_columns(folded, rows=n, dims=(3,))
        check(lib().h2r_fold_columns(self.chip._ctx, cols.data_ptr(), cols.stride(0), cols.stride(1), C, n, s.data_ptr(), batch, folded.data_ptr(),
                                     folded.stride(0), ptr(status), self.chip._stream()), "h2r_fold_columns")
        hold(self, "fold", s, cols, folded, status)
        return folded, status

    def _open_args(self, columns, points, where: str):
        """(cfg, descriptors, Q, points int64 [batch, num_points, 4] on the device) of `columns` = [(tensor, point_mask)], tensors uint8
        [batch, n, 32] per circuit or [n, 32] for a key column, and `points` = [batch][num_points] integers in the chip's representation."""
        batch, num_points, dev = len(points), len(points[0]), columns[0][0].device
        if not 0 < len(columns) <= _lib.H2R_OPEN_MAX_COLUMNS:
            check(_lib.H2R_E_SHAPE, where)
        n = columns[0][0].shape[-2]
        cfg = _lib.H2ROpenConfig(struct_size=ctypes.sizeof(_lib.H2ROpenConfig), n_coeffs=n, num_cols=len(columns), num_points=num_points)
        desc = (_lib.H2ROpenColumn * len(columns))()
        for d, (t, mask) in zip(desc, columns):
            assert is_columns(t, rows=n, dims=(2, 3), batch=batch)
            (d.base, d.elem_stride, _), d.point_mask = column_group(t, t.dim() == 3), int(mask)
        Q = int(lib().h2r_open_queries(ctypes.byref(cfg), desc, None))
        if Q == 0:
            check(_lib.H2R_E_SHAPE, "h2r_open_queries")
        pts = challenges(points, dev)
        assert pts.dim() == 3 and 0 < pts.shape[1] <= _lib.H2R_OPEN_MAX_POINTS
        return cfg, desc, Q, pts

    def open_eval(self, columns, points, out=None):
        """(evals, status): evals int64 [batch, Q, 4], the evaluations of columns in coefficient form at per-circuit points
        (h2r_open_eval_columns; halo2's eval_polynomial), in the chip's representation.
        columns: a list of (tensor, point_mask) in the caller's transcript order, tensors uint8 [batch, n, 32], or [n, 32] for a proving-key
        column shared by the batch; bit p of point_mask = "queried at points[e][p]".  The Q queries are the set bits in column order, points
        ascending within a column.  points: [batch][num_points] integers in the chip's representation (the caller forms the rotations of
        x).  status H2R_E_SHAPE where a point is not canonical (that circuit's evaluations are left untouched).  out: (evals, status) to
        write into (a status byte that is nonzero on entry skips the circuit; the call never clears it)."""
        cfg, desc, Q, pts = self._open_args(columns, points, "EvaluationDomain.open_eval")
        batch, dev = pts.shape[0], pts.device
        evals, status = outputs(out, dev, (torch.zeros, torch.int64, (batch, Q, 4)), status=batch)
        assert evals.is_contiguous() and tuple(evals.shape) == (batch, Q, 4)
        ws = workspace(lib().h2r_open_workspace_bytes(ctypes.byref(cfg), desc, batch), dev)
        check(lib().h2r_open_eval_columns(self.chip._ctx, ctypes.byref(cfg), desc, pts.data_ptr(), batch, evals.data_ptr(), ptr(status),
                                          ws.data_ptr(), self.chip._stream()), "h2r_open_eval_columns")
        hold(self, "open_eval", pts, ws, [t for t, _ in columns], evals, status)
        return evals, status

    def open_witness(self, columns, points, vs: Sequence[int], out=None):
        """(W, batch_evals, status): the witness polynomials of the GWC multi-open (h2r_open_witness_columns; kate_division of
        sum_i v^i f_i by X - z per point).  W uint8 [batch, num_points, n, 32]: per point the n coefficients of the
        quotient (the last one 0), over the columns whose mask names the point, in column order, the powers of v from v^0 for every point; a
        point that no column queries is left as it was (zeros when the call allocates).  batch_evals int64 [batch, num_points, 4]: the
        remainders sum v^idx f_c(z).  columns / points as open_eval; vs: per circuit, integers in the chip's representation.  status
        H2R_E_SHAPE where a point or v is not canonical.  out: (W, batch_evals, status) to write into (W must overlap no column)."""
        cfg, desc, _, pts = self._open_args(columns, points, "EvaluationDomain.open_witness")
        (batch, num_points), n, dev = pts.shape[:2], cfg.n_coeffs, pts.device
        v = challenges(vs, dev, batch)
        W, be, status = outputs(out, dev, (torch.zeros, torch.uint8, (batch, num_points, n, 32)), (torch.zeros, torch.int64, (batch, num_points, 4)), status=batch)
        assert is_columns(W, rows=n, dims=(4,)) and W.shape[1] == num_points
        assert be is None or (be.is_contiguous() and tuple(be.shape) == (batch, num_points, 4))
        ws = workspace(lib().h2r_open_workspace_bytes(ctypes.byref(cfg), desc, batch), dev)
        check(lib().h2r_open_witness_columns(self.chip._ctx, ctypes.byref(cfg), desc, pts.data_ptr(), v.data_ptr(), batch, W.data_ptr(), W.stride(0),
                                             W.stride(1), ptr(be), ptr(status), ws.data_ptr(), self.chip._stream()), "h2r_open_witness_columns")
        hold(self, "open_witness", pts, v, ws, [t for t, _ in columns], W, be, status)
        return W, be, status


class CommitKey:
    """The bases of the commitments on the device (h2r_msm_columns): n affine points of the curve of the chip's field
    (bn256 G1 for bn254_fr; every other field is refused), 64 bytes each -- x then y, Fq elements in the chip's representation, (0, 0) the
    identity -- as halo2curves' `ParamsKZG::g` / `g_lagrange` lie in memory for a Montgomery chip.  The bases are not validated."""

    def __init__(self, chip: "BigIntChip", bases: torch.Tensor):
        words_form = bases.dtype == torch.int64 and bases.dim() == 3 and tuple(bases.shape[1:]) == (2, 4)
        if not words_form and not (bases.dtype == torch.uint8 and bases.dim() == 2 and bases.shape[1] == 64):
            check(_lib.H2R_E_SHAPE, "CommitKey")
        assert bases.is_contiguous() and bases.is_cuda
        self.chip, self.bases, self.n = chip, bases, int(bases.shape[0])

    def _config(self, num_cols: int):
        return _lib.H2RMsmConfig(struct_size=ctypes.sizeof(_lib.H2RMsmConfig), n=self.n, num_cols=num_cols, reserved=0)

    def _workspace(self, given, need: int):
        """The caller's workspace, or a new one of `need` bytes."""
        ws = given if given is not None else workspace(need, self.bases.device)
        assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= need
        return ws

    def plan(self, num_cols: int, batch: int) -> "_lib.H2RMsmInfo":
        """window_bits, num_windows, slice_points, num_slices and workspace_bytes of a call (h2r_msm_plan, a host function)."""
        info, cfg = _lib.H2RMsmInfo(), self._config(num_cols)
        if lib().h2r_msm_plan(ctypes.byref(cfg), batch, ctypes.byref(info)) == 0:
            check(_lib.H2R_E_SHAPE, "h2r_msm_plan")
        return info

    def commit(self, columns, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int64 [batch, num_cols, 2, 4]: the affine commitments sum_i columns[c][e][i] * bases[i] in the chip's representation, (0, 0) for the
        identity.  columns: a list of tensors uint8 [batch, n, 32] (scalars in the chip's representation), or [n, 32] for a column the
        whole batch shares (batch = 1 where every column is such a one).  out: the tensor to write into (it must overlap no input);
        status: uint8 [batch], a byte that is nonzero on entry skips the circuit (its commitments are left as they were); workspace: uint8,
        plan(num_cols, batch).workspace_bytes bytes, 16-byte aligned, the call's own until the stream has run it (allocated when None)."""
        if not 0 < len(columns) <= _lib.H2R_MSM_MAX_COLUMNS:
            check(_lib.H2R_E_SHAPE, "CommitKey.commit")
        batch = next((int(t.shape[0]) for t in columns if t.dim() == 3), 1)
        cfg = self._config(len(columns))
        desc = (_lib.H2RMsmColumn * len(columns))()
        for d, t in zip(desc, columns):
            assert is_columns(t, rows=self.n, dims=(2, 3), batch=batch)
            d.base, d.elem_stride, _ = column_group(t, t.dim() == 3)
        out = outputs(out, self.bases.device, (torch.zeros, torch.int64, (batch, len(columns), 2, 4)))
        assert out.is_contiguous() and out.dtype == torch.int64 and tuple(out.shape) == (batch, len(columns), 2, 4)
        ws = self._workspace(workspace, int(lib().h2r_msm_workspace_bytes(ctypes.byref(cfg), batch)))
        check(lib().h2r_msm_columns(self.chip._ctx, ctypes.byref(cfg), desc, self.bases.data_ptr(), batch, out.data_ptr(), ptr(status),
                                    ws.data_ptr(), self.chip._stream()), "h2r_msm_columns")
        hold(self, "commit", ws, list(columns), out, status)
        return out

    def transform(self, omega: int, k: Optional[int] = None, inverse: bool = True, out: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None) -> "CommitKey":
        """A new key over the transform of the first 2^k bases (h2r_curve_ntt): inverse (the default)
        out[i] = [n^-1] sum_j [omega^(-i j)] bases[j] -- with the powers of tau as bases and the domain's omega, halo2's g_lagrange --,
        forward out[i] = sum_j [omega^(i j)] bases[j].  omega: a primitive 2^k-th root of unity of the chip's field, an integer in the chip's
        representation.  k: log2 n by default; a key whose n is no power of two needs an explicit k <= log2 n.  out: the tensor of 2^k
        points to write into (the layout of `bases`; it must overlap neither the bases nor the workspace); workspace: uint8,
        h2r_curve_ntt_workspace_bytes bytes, 16-byte aligned, the call's own until the stream has run it (allocated when None)."""
        if k is None:
            k = self.n.bit_length() - 1
            if self.n != 1 << k:
                check(_lib.H2R_E_SHAPE, "CommitKey.transform")
        k = int(k)
        if k < 1 or (1 << k) > self.n:
            check(_lib.H2R_E_SHAPE, "CommitKey.transform")
        cfg = _lib.H2RCurveNttConfig(struct_size=ctypes.sizeof(_lib.H2RCurveNttConfig), log_n=k, flags=_lib.H2R_CURVE_NTT_INVERSE if inverse else 0, reserved=0)
        set_words(cfg.omega, omega)
        n = 1 << k
        out = outputs(out, self.bases.device, (torch.zeros, torch.int64, (n, 2, 4)) if self.bases.dtype == torch.int64 else (torch.zeros, torch.uint8, (n, 64)))
        assert out.is_contiguous() and out.is_cuda and out.numel() * out.element_size() == 64 * n
        ws = self._workspace(workspace, int(lib().h2r_curve_ntt_workspace_bytes(ctypes.byref(cfg))))
        check(lib().h2r_curve_ntt(self.chip._ctx, ctypes.byref(cfg), self.bases.data_ptr(), out.data_ptr(), ws.data_ptr(), self.chip._stream()),
              "h2r_curve_ntt")
        key = CommitKey(self.chip, out)
        hold(key, "transform", ws, self.bases, out)
        return key


def random_columns(chip: "BigIntChip", columns, tags: Sequence[int], rows, seed: bytes, first_circuit: int = 0) -> None:
    """Fills rows [rows[0], rows[1]) of every column with uniform field elements drawn from `seed` (h2r_random_columns; DESIGN.md section
    2m): element(seed, circuit, tag, row) = BLAKE2b-512(person "H2R-Blinding-v1\\0", seed | le64(circuit) | le32(tag) | le32(0) | le64(row))
    as a little-endian integer modulo r, in the chip's representation -- the same values whatever the representation and however a batch
    or a row range is cut into calls.  columns: up to 64 tensors uint8 [batch, n, 32] (circuit e draws with index first_circuit + e), or
    [n, 32] for a column the batch shares (drawn once, with index first_circuit), last two dimensions contiguous; tags: one integer per
    column (the caller's table of column kinds); seed: 32 bytes, passed by value.  Nothing but the named rows is written; the columns'
    ranges are the caller's to keep apart.  Only a chip whose field has a curve (bn254_fr)."""
    columns, tags, (row_begin, row_end) = list(columns), list(tags), rows
    if not 0 < len(columns) <= _lib.H2R_RANDOM_MAX_COLUMNS or len(tags) != len(columns) or len(seed) != 32 or not 0 <= row_begin <= row_end:
        check(_lib.H2R_E_SHAPE, "random_columns")
    batch = next((int(t.shape[0]) for t in columns if t.dim() == 3), 1)
    cfg = _lib.H2RRandomConfig(struct_size=ctypes.sizeof(_lib.H2RRandomConfig), num_cols=len(columns), row_begin=row_begin, row_end=row_end,
                               first_circuit=first_circuit, reserved=0)
    cfg.seed[:] = bytes(seed)
    desc = (_lib.H2RRandomColumn * len(columns))()
    for d, t, tag in zip(desc, columns, tags):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and is_columns(t, dims=(2, 3), batch=batch) and t.shape[-2] >= row_end):
            check(_lib.H2R_E_SHAPE, "random_columns")     # (no assert: a column shorter than row_end must never reach the kernel)
        (d.base, d.elem_stride, _), d.tag = column_group(t, t.dim() == 3), int(tag)
    check(lib().h2r_random_columns(chip._ctx, ctypes.byref(cfg), desc, batch, chip._stream()), "h2r_random_columns")


class Transcript:
    """halo2's Fiat-Shamir transcript for a batch of circuits on the device (h2r_transcript_round):
    `Blake2bWrite<_, G1Affine, Challenge255<_>>`, one launch per round, no host synchronisation between the stages.  Owns the per-circuit
    states and the proof buffer uint8 [batch, proof_bytes] (proof_bytes a multiple of 32) and keeps the running write offset: a round
    writes 32 bytes per written item, the same for every circuit.  Only a chip whose field has a curve (bn254_fr)."""

    POINT, SCALAR = "point", "scalar"

    def __init__(self, chip: "BigIntChip", batch: int, proof_bytes: int):
        if batch < 1 or proof_bytes < 0 or proof_bytes % 32:
            check(_lib.H2R_E_SHAPE, "Transcript")
        dev = "cuda:%d" % chip.device
        self.chip, self.batch, self.offset, self.started = chip, int(batch), 0, False
        self.states = torch.zeros((batch, int(lib().h2r_transcript_state_bytes())), dtype=torch.uint8, device=dev)
        # (a transcript that only draws challenges has proof_bytes = 0: its rows still get a 16-byte aligned stride)
        self.buffer = torch.zeros((batch, max(int(proof_bytes), 32)), dtype=torch.uint8, device=dev)[:, :proof_bytes]

    def _item(self, item, common: bool) -> "_lib.H2RTranscriptItem":
        """A tensor, or (tensor, POINT | SCALAR), as a descriptor.  Points: int64 [batch, count, 2, 4] or uint8 [batch, count, 64] per
        circuit; with a kind also int64 [count, 2, 4] / [2, 4] or uint8 [count, 64] / [64] for one copy the batch shares.  Scalars: int64
        [batch, count, 4] or uint8 [batch, count, 32] per circuit, int64 [count, 4] / [4] or uint8 [count, 32] / [32] shared.  Without a
        kind the dimensions decide: int64 with four is points, uint8 by its last dimension, everything else scalars."""
        t, kind = item if isinstance(item, (tuple, list)) else (item, None)
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.int64, torch.uint8) or t.dim() == 0:
            check(_lib.H2R_E_SHAPE, "Transcript.round")
        words_form = t.dtype == torch.int64
        if kind is None:
            kind = self.POINT if (words_form and t.dim() == 4) or (not words_form and t.shape[-1] == 64) else self.SCALAR
        tail = ((2, 4) if kind == self.POINT else (4,)) if words_form else ((64,) if kind == self.POINT else (32,))
        lead = t.dim() - len(tail)
        if kind not in (self.POINT, self.SCALAR) or lead not in (0, 1, 2) or tuple(t.shape[lead:]) != tail or (lead == 2 and t.shape[0] != self.batch):
            check(_lib.H2R_E_SHAPE, "Transcript.round")
        count = int(t.shape[lead - 1]) if lead else 1
        assert t[0].is_contiguous() if lead == 2 else t.is_contiguous(), "the entries of an item lie back to back"
        d = _lib.H2RTranscriptItem()
        d.base, d.elem_stride, d.count = t.data_ptr(), t.stride(0) * t.element_size() if lead == 2 else 0, count
        d.kind, d.flags = _lib.H2R_TRANSCRIPT_POINT if kind == self.POINT else _lib.H2R_TRANSCRIPT_SCALAR, _lib.H2R_TRANSCRIPT_COMMON if common else 0
        return d

    def round(self, items=(), squeeze: int = 0, derive=(), common: bool = False, status: Optional[torch.Tensor] = None, out=None):
        """(challenges, derived): int64 [batch, squeeze, 4] and int64 [batch, len(derive), 4] on the device, in the chip's representation
        -- every stage method takes them (or a view such as challenges[:, 0]) for its thetas, betas, gammas, ys, scalars, points and vs.
        items: tensors (see _item) absorbed in order and, unless `common`, appended to the proof; derive: (src, mult, log2_pow) triples,
        derived[e][j] = mult * challenges[e][src]^(2^log2_pow), mult an integer in the chip's representation (x * omega^rot for the opening
        points, x^n for the fold).  status: uint8 [batch]; a byte that is nonzero on entry skips the circuit (state, proof and outputs
        untouched; the call never clears it), H2R_E_ASSERTION marks a (0, 0) point, H2R_E_SHAPE a value that is not canonical.  out:
        (challenges, derived) to write into.  The first round initialises the states."""
        items, derive, dev = list(items), list(derive), self.states.device
        if len(items) > _lib.H2R_TRANSCRIPT_MAX_ITEMS or not 0 <= squeeze <= _lib.H2R_TRANSCRIPT_MAX_SQUEEZE or len(derive) > _lib.H2R_TRANSCRIPT_MAX_DERIVE:
            check(_lib.H2R_E_SHAPE, "Transcript.round")
        cfg = _lib.H2RTranscriptConfig(struct_size=ctypes.sizeof(_lib.H2RTranscriptConfig), num_items=len(items), num_squeeze=squeeze,
                                       num_derive=len(derive), flags=0 if self.started else _lib.H2R_TRANSCRIPT_INIT, reserved=0)
        desc = (_lib.H2RTranscriptItem * max(len(items), 1))(*[self._item(it, common) for it in items])
        dv = (_lib.H2RTranscriptDerive * max(len(derive), 1))()
        for d, (src, mult, log2_pow) in zip(dv, derive):
            d.src, d.log2_pow = int(src), int(log2_pow)
            set_words(d.mult, mult)
        nbytes = 0 if common else 32 * sum(int(d.count) for d in desc[:len(items)])
        if self.offset + nbytes > self.buffer.shape[1]:
            check(_lib.H2R_E_SHAPE, "Transcript.round")
        challenges_out, derived = outputs(out, dev, (torch.zeros, torch.int64, (self.batch, squeeze, 4)), (torch.zeros, torch.int64, (self.batch, len(derive), 4)))
        for t, n in ((challenges_out, squeeze), (derived, len(derive))):
            assert t.is_contiguous() and t.dtype == torch.int64 and tuple(t.shape) == (self.batch, n, 4)
        check(lib().h2r_transcript_round(self.chip._ctx, ctypes.byref(cfg), desc if items else None, dv if derive else None, self.states.data_ptr(),
                                         self.batch, challenges_out.data_ptr() if squeeze else None, derived.data_ptr() if derive else None,
                                         self.buffer.data_ptr() if nbytes else None, self.buffer.stride(0), self.offset, ptr(status), self.chip._stream()),
              "h2r_transcript_round")
        self.started, self.offset = True, self.offset + nbytes
        hold(self, "round", [it[0] if isinstance(it, (tuple, list)) else it for it in items], challenges_out, derived, status)
        return challenges_out, derived

    def write_points(self, points: torch.Tensor, squeeze: int = 0, derive=(), status: Optional[torch.Tensor] = None):
        """Absorbs and writes points (CommitKey.commit's output as it is); round()'s return."""
        return self.round([(points, self.POINT)], squeeze, derive, False, status)

    def write_scalars(self, scalars: torch.Tensor, squeeze: int = 0, derive=(), status: Optional[torch.Tensor] = None):
        """Absorbs and writes scalars (open_eval's evaluations as they are); round()'s return."""
        return self.round([(scalars, self.SCALAR)], squeeze, derive, False, status)

    def common_points(self, points: torch.Tensor, squeeze: int = 0, derive=(), status: Optional[torch.Tensor] = None):
        """Absorbs points without writing them; round()'s return."""
        return self.round([(points, self.POINT)], squeeze, derive, True, status)

    def common_scalars(self, scalars: torch.Tensor, squeeze: int = 0, derive=(), status: Optional[torch.Tensor] = None):
        """Absorbs scalars without writing them (the verifying key's digest, the instances); round()'s return."""
        return self.round([(scalars, self.SCALAR)], squeeze, derive, True, status)

    def proof(self) -> torch.Tensor:
        """uint8 [batch, offset]: the proof bytes written so far (a view of the buffer)."""
        return self.buffer[:, :self.offset]


# column kind x index of the generator's tags: tag = kind * 256 + index
TAG_ADVICE, TAG_LOOKUP_A_PERM, TAG_LOOKUP_S_PERM, TAG_PERM_Z, TAG_LOOKUP_Z, TAG_RANDOM_POLY = (kind * 256 for kind in range(6))


class ProvingKey:
    """What create_proof needs of one circuit shape, built once and held on the device: the domain, the monomial and
    the Lagrange CommitKey, the fixed and sigma columns in Lagrange, coefficient and extended form, vanishing_columns, the row kinds, the
    lookup, permutation and quotient configurations, first_row, the image's rows, the number of h pieces and the caller's vk_repr.
    fixed: uint8 [F, 2^k, 32], sigma: uint8 [m, 2^k, 32], Lagrange form, the chip's representation; kinds: the image's row kinds; delta and
    vk_repr: integers in the chip's representation (keygen() below builds all four from the circuit).  commit_key: the monomial key, at
    least 2^k bases; lagrange_key: dom.lagrange_key(commit_key) when None."""

    def __init__(self, chip, dom: EvaluationDomain, commit_key: CommitKey, la: LookupArgument, fixed: torch.Tensor, sigma: torch.Tensor, kinds,
                 blinding_factors: int, delta: int, gate_fixed: Sequence[int], column_src: Sequence[int], chunk_len: int, lookup_advice: Sequence[int],
                 lookup_tag: Sequence[int], lookup_enable: Sequence[int], table_tag: int, table_value: int, vk_repr: int, first_row: int = 0,
                 lookup_mask: int = 31, h_pieces: int = 4, lagrange_key: Optional[CommitKey] = None):
        n = 1 << dom.k
        dev = fixed.device
        if (h_pieces != 4 or dom.extended_k != dom.k + 3 or commit_key.n < n or not is_columns(fixed, rows=n, dims=(3,)) or not is_columns(sigma, rows=n, dims=(3,))
                or sigma.shape[0] != len(column_src) or any(int(s) >= 5 for s in column_src) or n - blinding_factors - 1 < 1):
            check(_lib.H2R_E_SHAPE, "ProvingKey")     # (four pieces: the constraint system's degree 5 at extended_k = k + 3; no extra columns)
        self.chip, self.dom, self.la, self.n, self.u, self.blinding_factors = chip, dom, la, n, n - blinding_factors - 1, int(blinding_factors)
        self.ck = commit_key if commit_key.n == n else CommitKey(chip, commit_key.bases[:n])
        self.lk = lagrange_key if lagrange_key is not None else dom.lagrange_key(self.ck)
        self.delta, self.gate_fixed, self.column_src, self.chunk_len = int(delta), list(gate_fixed), list(column_src), int(chunk_len)
        self.lookup = dict(lookup_mask=lookup_mask, lookup_advice=list(lookup_advice), lookup_tag=list(lookup_tag), lookup_enable=list(lookup_enable),
                           table_tag=int(table_tag), table_value=int(table_value))
        self.lookup_args = [a for a in range(LookupArgument.ARGS) if (lookup_mask >> a) & 1]
        if self.lookup_args != list(range(LookupArgument.ARGS)):
            check(_lib.H2R_E_SHAPE, "ProvingKey")     # (the lookup stages' wrappers pack all five arguments)
        self.pa = PermutationArgument(chip, column_src, chunk_len, delta, dom.omega)
        self.h_pieces, self.first_row = int(h_pieces), int(first_row)
        self.kinds = kinds_tensor(kinds, dev)
        self.rows = int(self.kinds.numel())
        self.fixed_lag, self.sigma_lag = fixed, sigma
        self.fixed_coeff, self.sigma_coeff = dom.lagrange_to_coeff(fixed), dom.lagrange_to_coeff(sigma)
        self.fixed_ext, self.sigma_ext = dom.coeff_to_extended(self.fixed_coeff), dom.coeff_to_extended(self.sigma_coeff)
        self.l_ext = dom.vanishing_columns(blinding_factors)
        self.vk = challenges([vk_repr], dev)
        # x * omega, x * omega^-(blinding_factors + 1), x * omega^-1 and x^n: the derived values of the round that draws x
        mont = chip.montgomery
        w = dom._field(_lib.FIELD_FROM_MONTGOMERY, dom.omega) if mont else dom.omega
        wi = dom._field(3, w)
        wl = wi
        for _ in range(blinding_factors):
            wl = dom._field(_lib.FIELD_MUL, wl, wi)
        rep = (lambda v: dom._field(_lib.FIELD_TO_MONTGOMERY, v)) if mont else (lambda v: v)
        self.derive = [(0, dom.omega, 0), (0, rep(wl), 0), (0, rep(wi), 0), (0, dom.one, dom.k)]
        S, A = self.pa.sets, self.lookup_args
        self.eval_plan, self.open_plan = _plans(fixed.shape[0], sigma.shape[0], S, A)
        self.num_evals = sum(bin(m).count("1") for _, _, m in self.eval_plan)
        self.proof_bytes = 32 * (5 + 2 * len(A) + S + len(A) + 1 + self.h_pieces + self.num_evals + 4)


def create_proof(key: ProvingKey, image: torch.Tensor, batch: int, seed: Optional[bytes] = None, instances: Optional[torch.Tensor] = None,
                 group: Optional[int] = None):
    """(proof uint8 [batch, key.proof_bytes], status uint8 [batch]): `batch` independent one-circuit proofs, each with its own transcript
    (unlike upstream's several circuits under one transcript), from the advice image to the proof bytes with no host synchronisation in
    between (DESIGN.md section 2m holds the round order).  image: the chip's advice image of key.rows rows per circuit, [batch, bytes];
    a planar image with col_stride = 2^k * 32 IS the advice columns and gets its rows u..n written in place.  seed: 32 bytes, os.urandom(32)
    when None -- A SEED REUSED WITH ANOTHER WITNESS REUSES THE BLINDING.  instances: int64 [batch, I, 4] on the device, absorbed as common
    scalars.  group: how many circuits' columns are alive at once (the whole batch when None); circuit e always draws with index e, so the
    proofs do not depend on it.  One status is threaded through every stage: a circuit that a stage flags is skipped by the later ones and
    ends with its code (H2R_E_ASSERTION where a grand product does not close: the image does not satisfy the circuit)."""
    chip, dom, la, n, u = key.chip, key.dom, key.la, key.n, key.u
    seed = os.urandom(32) if seed is None else bytes(seed)
    if batch < 1 or len(seed) != 32 or image.dim() != 2 or image.shape[0] != batch or (group is not None and group < 1):
        check(_lib.H2R_E_SHAPE, "create_proof")
    dev, A, S, fr, rows, N = image.device, len(key.lookup_args), key.pa.sets, key.first_row, key.rows, 1 << dom.extended_k
    planar = bool(getattr(chip, "columns", False))
    if (planar and (image.shape[1] != 5 * n * 32 or getattr(chip, "col_stride", 0) != n * 32)) or (not planar and image.shape[1] != rows * 160) or fr + rows > u:
        check(_lib.H2R_E_SHAPE, "create_proof")
    proof = torch.zeros((batch, key.proof_bytes), dtype=torch.uint8, device=dev)
    status = torch.zeros(batch, dtype=torch.uint8, device=dev)
    group = batch if group is None else min(int(group), batch)

    def zeros(*shape):
        return torch.zeros(shape + (32,), dtype=torch.uint8, device=dev)

    def split(t):
        return [t[:, c] for c in range(t.shape[1])]

    def tags(base, count):
        return [base + i for i in range(count)]

    for g0 in range(0, batch, group):
        B = min(group, batch - g0)
        img, st = image[g0:g0 + B], status[g0:g0 + B]
        tr = Transcript(chip, B, key.proof_bytes)
        # 1. the verifying key and the instances
        tr.round([(key.vk, tr.SCALAR)] + ([(instances[g0:g0 + B], tr.SCALAR)] if instances is not None and instances.shape[1] else []), common=True, status=st)
        # 2. advice: rows u..n from the generator, committed in Lagrange form; theta
        if planar:
            adv = img.view(B, 5, n, 32)
        else:
            adv = zeros(B, 5, n)
            adv[:, :, fr:fr + rows] = img.view(B, rows, 5, 32).permute(0, 2, 1, 3)
        random_columns(chip, split(adv), tags(TAG_ADVICE, 5), (u, n), seed, first_circuit=g0)
        theta = tr.write_points(key.lk.commit(split(adv), status=st), squeeze=1, status=st)[0][:, 0]
        # 3. the lookups' A' and S'; beta, gamma
        hist = la.hist_advice(key.kinds, img, B, la.new_hist(B), status=st)
        a_perm, s_perm, st_perm = la.permuted_columns(hist, theta, u)
        st.copy_(torch.where(st == 0, st_perm, st))
        a_in = la.input_columns(key.kinds, img, B, theta, u, status=st, first_row=fr)
        AP, SP = zeros(B, la.ARGS, n), zeros(B, la.ARGS, n)
        AP[:, :, :u], SP[:, :, :u] = a_perm, s_perm
        random_columns(chip, split(AP) + split(SP), tags(TAG_LOOKUP_A_PERM, A) + tags(TAG_LOOKUP_S_PERM, A), (u, n), seed, first_circuit=g0)
        pairs = [t[:, a] for a in range(A) for t in (AP, SP)]
        bg = tr.write_points(key.lk.commit(pairs, status=st), squeeze=2, status=st)[0]
        beta, gamma = bg[:, 0], bg[:, 1]
        # 4. both families of Z and the random polynomial; y
        PZ, LZ, RP = zeros(B, S, n), zeros(B, la.ARGS, n), zeros(B, n)
        key.pa.product_columns(img, B, rows, key.sigma_lag, beta, gamma, u, first_row=fr, out=(PZ, st))
        lz, _ = la.product_columns(a_in, a_perm, s_perm, theta, beta, gamma, u, out=(zeros(B, la.ARGS, u + 1), st))
        LZ[:, :, :u + 1] = lz
        random_columns(chip, split(PZ) + split(LZ), tags(TAG_PERM_Z, S) + tags(TAG_LOOKUP_Z, A), (u + 1, n), seed, first_circuit=g0)
        random_columns(chip, [RP], [TAG_RANDOM_POLY], (0, n), seed, first_circuit=g0)
        y = tr.round([(key.lk.commit(split(PZ) + split(LZ), status=st), tr.POINT), (key.ck.commit([RP], status=st), tr.POINT)], squeeze=1, status=st)[0][:, 0]
        # 5. the quotient and its pieces; x, its rotations and x^n
        coeff = {name: dom.lagrange_to_coeff(t) for name, t in (("advice", adv), ("perm_z", PZ), ("lookup_a_perm", AP), ("lookup_s_perm", SP), ("lookup_z", LZ))}
        ext = {name: dom.coeff_to_extended(t) for name, t in coeff.items()}
        h, _ = dom.quotient(key.blinding_factors, key.delta, key.gate_fixed, key.column_src, key.chunk_len, ext["advice"], ext["perm_z"], key.fixed_ext,
                            key.sigma_ext, key.l_ext, theta, beta, gamma, y, lookup_a_perm=ext["lookup_a_perm"], lookup_s_perm=ext["lookup_s_perm"],
                            lookup_z=ext["lookup_z"], out=(zeros(B, N), st), **key.lookup)
        del ext
        pieces = dom.extended_to_coeff(h)[:, :key.h_pieces * n].unflatten(1, (key.h_pieces, n))
        xs, dv = tr.write_points(key.ck.commit(split(pieces), status=st), squeeze=1, derive=key.derive, status=st)
        points, xn = torch.cat([xs, dv[:, :3]], dim=1), dv[:, 3]
        # 6. the evaluations, in transcript order; v
        coeff["random"], coeff["fixed"], coeff["sigma"] = RP.unsqueeze(1), key.fixed_coeff, key.sigma_coeff
        coeff["h"] = dom.fold(pieces, xn, out=(zeros(B, n), st))[0].unsqueeze(1)

        def columns(plan):
            return [(coeff[g][i] if g in ("fixed", "sigma") else coeff[g][:, i], mask) for g, i, mask in plan]

        evals, _ = dom.open_eval(columns(key.eval_plan), points, out=(torch.zeros((B, key.num_evals, 4), dtype=torch.int64, device=dev), st))
        v = tr.write_scalars(evals, squeeze=1, status=st)[0][:, 0]
        # 7. the GWC witness polynomials
        W, _, _ = dom.open_witness(columns(key.open_plan), points, v, out=(zeros(B, 4, n), torch.zeros((B, 4, 4), dtype=torch.int64, device=dev), st))
        tr.write_points(key.ck.commit(split(W), status=st), status=st)
        proof[g0:g0 + B] = tr.proof()
    return proof, status


# ---- the verifier up to the pairing -----------------------------------------------------------------------------------
TAG_COMBINE = 6 * 256                      # the generator's tag of combine's rho: kind 6, one row per circuit


def _plans(num_fixed: int, num_sigma: int, sets: int, lookup_args):
    """(eval_plan, open_plan): the evaluations in transcript order and the GWC query list, as (group, index, point mask); the point sets
    are x, omega x, omega^-(bf+1) x, omega^-1 x."""
    adv = [("advice", c, 3 if c == 4 else 1) for c in range(5)]
    fx, sg = [("fixed", i, 1) for i in range(num_fixed)], [("sigma", c, 1) for c in range(num_sigma)]
    pz = [("perm_z", s, 3 | (4 if s < sets - 1 else 0)) for s in range(sets)]
    lk = [q for a in lookup_args for q in (("lookup_z", a, 3), ("lookup_a_perm", a, 9), ("lookup_s_perm", a, 1))]
    return adv + fx + [("random", 0, 1)] + sg + pz + lk, adv + pz + lk + fx + sg + [("h", 0, 1), ("random", 0, 1)]


def _points_tensor(t, count: int, dev) -> torch.Tensor:
    """uint8 [count, 64] on `dev` of points given as int64 [..., count, 2, 4] / [2, 4] or uint8 [..., count, 64] / [64]."""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int64, torch.uint8) or t.numel() * t.element_size() != 64 * count:
        check(_lib.H2R_E_SHAPE, "VerifyingKey")
    return t.to(dev).contiguous().view(torch.uint8).reshape(count, 64)


class VerifyingKey:
    """What verify_proof needs of one circuit shape, held on the device: the constraint system's configuration and
    the two plans (h2r_verify_scalars' config), the proof's section list, the commitments of the fixed and sigma columns followed by G --
    the key's tail of the base order --, and the caller's vk_repr.  Constructible from commitments alone: a verifier holds no columns.
    dom: the EvaluationDomain (k, omega); fixed_commitments / sigma_commitments: F and m affine points (int64 [F, 2, 4] or uint8 [F, 64],
    a leading batch dimension of 1 is taken as it comes from CommitKey.commit); g: the commit key's first base; delta, vk_repr: integers
    in the chip's representation.  ProvingKey.verifying_key() builds one from a proving key."""

    def __init__(self, chip, dom: EvaluationDomain, fixed_commitments: torch.Tensor, sigma_commitments: torch.Tensor, g: torch.Tensor, blinding_factors: int,
                 delta: int, gate_fixed: Sequence[int], column_src: Sequence[int], chunk_len: int, lookup_advice: Sequence[int], lookup_tag: Sequence[int],
                 lookup_enable: Sequence[int], table_tag: int, table_value: int, vk_repr: int, lookup_mask: int = 31, h_pieces: int = 4):
        dev = "cuda:%d" % chip.device
        F, m = int(fixed_commitments.numel() * fixed_commitments.element_size() // 64), len(column_src)
        if (h_pieces != 4 or len(gate_fixed) != 9 or not 0 < m <= _lib.H2R_PERM_MAX_COLUMNS or chunk_len < 1 or
                any(len(x) != _lib.H2R_LOOKUP_ARGS for x in (lookup_advice, lookup_tag, lookup_enable))):
            check(_lib.H2R_E_SHAPE, "VerifyingKey")
        self.chip, self.dom, self.h_pieces = chip, dom, 4
        self.lookup_args = [a for a in range(LookupArgument.ARGS) if (lookup_mask >> a) & 1]
        chunk = min(int(chunk_len), m)
        S, A = (m + chunk - 1) // chunk, len(self.lookup_args)
        self.eval_plan, self.open_plan = _plans(F, m, S, self.lookup_args)
        self.cfg = cfg = _lib.H2RVerifyScalarsConfig(struct_size=ctypes.sizeof(_lib.H2RVerifyScalarsConfig), log_n=dom.k, blinding_factors=blinding_factors,
                                                     num_fixed=F, num_columns=m, chunk_len=chunk_len, lookup_mask=lookup_mask,
                                                     num_eval_plan=len(self.eval_plan), num_open_plan=len(self.open_plan), reserved=0)
        if max(len(self.eval_plan), len(self.open_plan)) > _lib.H2R_VERIFY_MAX_PLAN:
            check(_lib.H2R_E_SHAPE, "VerifyingKey")
        set_words(cfg.omega, dom.omega)
        set_words(cfg.delta, delta)
        for i, v in enumerate(gate_fixed):
            cfg.gate_fixed[i] = int(v)
        for c, s in enumerate(column_src):
            cfg.column_src[c] = int(s)
        for k in range(_lib.H2R_LOOKUP_ARGS):
            cfg.lookup_advice[k], cfg.lookup_tag[k], cfg.lookup_enable[k] = int(lookup_advice[k]), int(lookup_tag[k]), int(lookup_enable[k])
        cfg.table_tag, cfg.table_value = int(table_tag), int(table_value)
        for table, plan in ((cfg.eval_plan, self.eval_plan), (cfg.open_plan, self.open_plan)):
            for entry, (group, index, mask) in zip(table, plan):
                entry.group, entry.index, entry.mask, entry.reserved = _lib.VERIFY_GROUPS.index(group), index, mask, 0
        num_evals = ctypes.c_uint32(0)
        self.num_bases = int(lib().h2r_verify_bases(ctypes.byref(cfg), ctypes.byref(num_evals)))
        if self.num_bases == 0:
            check(_lib.H2R_E_SHAPE, "h2r_verify_bases")
        self.num_evals = int(num_evals.value)
        # the proof's sections, in order: (name, kind, count)
        self.sections = [("advice", Transcript.POINT, 5), ("lookup_perm", Transcript.POINT, 2 * A), ("perm_z", Transcript.POINT, S),
                         ("lookup_z", Transcript.POINT, A), ("random", Transcript.POINT, 1), ("h", Transcript.POINT, self.h_pieces),
                         ("evals", Transcript.SCALAR, self.num_evals), ("w", Transcript.POINT, 4)]
        self.sections = [s for s in self.sections if s[2]]
        self.num_points = sum(c for _, kind, c in self.sections if kind == Transcript.POINT)
        self.proof_bytes = 32 * (self.num_points + self.num_evals)
        self.w_pos = self.num_points - 4
        assert self.num_bases == self.num_points + F + m + 1
        self.key_bases = torch.cat([_points_tensor(fixed_commitments, F, dev), _points_tensor(sigma_commitments, m, dev), _points_tensor(g, 1, dev)])
        self.vk = challenges([vk_repr], dev)


def _key_commitments(lk: CommitKey, fixed: torch.Tensor, sigma: torch.Tensor):
    """The commitments of the fixed and the sigma columns with the Lagrange key: int64 [1, F, 2, 4] and [1, m, 2, 4]."""
    return lk.commit([fixed[i] for i in range(fixed.shape[0])]), lk.commit([sigma[c] for c in range(sigma.shape[0])])


def _verifying_key(self: ProvingKey) -> VerifyingKey:
    """The verifying half of this key: the commitments of the fixed and sigma columns, formed once with the Lagrange key (a key that
    keygen() made keeps the ones it formed)."""
    if getattr(self, "commitments", None) is None:
        self.commitments = _key_commitments(self.lk, self.fixed_lag, self.sigma_lag)
    fixed, sigma = self.commitments
    return VerifyingKey(self.chip, self.dom, fixed, sigma, self.ck.bases[0],self.blinding_factors, self.delta, self.gate_fixed, self.column_src, self.chunk_len,
                        self.lookup["lookup_advice"], self.lookup["lookup_tag"], self.lookup["lookup_enable"], self.lookup["table_tag"],
                        self.lookup["table_value"], from_words(self.vk[0].tolist()), lookup_mask=self.lookup["lookup_mask"], h_pieces=self.h_pieces)


ProvingKey.verifying_key = _verifying_key


# ---- key generation --------------------------------------------------------------------------------------------------
# The constraint system of an advice image: fixed columns 0..8 the gate selectors in h2r_fixed_row's order, then the table's tag and value,
# the composition arguments' tag / enable, the overflow argument's tag / enable (h2r_keygen_fixed_columns' order).
NUM_FIXED = _lib.H2R_KEYGEN_NUM_FIXED
GATE_FIXED = tuple(range(9))
F_TABLE_TAG, F_TABLE_VALUE, F_COMP_TAG, F_COMP_ENABLE, F_OVER_TAG, F_OVER_ENABLE = 9, 10, 11, 12, 13, 14
LOOKUP_ADVICE = (0, 1, 2, 3, 0)                      # composition_a..d read columns a..d, overflow_a column a
LOOKUP_TAG = (F_COMP_TAG,) * 4 + (F_OVER_TAG,)
LOOKUP_ENABLE = (F_COMP_ENABLE,) * 4 + (F_OVER_ENABLE,)


def field_delta(chip) -> int:
    """delta of the chip's field (halo2's: a generator of the odd-order subgroup), in the chip's representation."""
    d = _lib.FIELD_DELTA[chip.field]
    if not chip.montgomery:
        return d
    wa, wb, out = ((ctypes.c_uint64 * 4)(*words(v)) for v in (d, 0, 0))
    check(lib().h2r_field_eval(chip._ctx, _lib.FIELD_TO_MONTGOMERY, wa, wb, out), "h2r_field_eval")
    return from_words(out)


def copy_pairs_tensor(pairs, dev) -> torch.Tensor:
    """int32 [n, 4] on the device: h2r_copy entries (row, col, src_row, src_col) from the ctypes array chip.pow_copy_map returns, from
    anything numpy takes as [n, 4] unsigned integers, or a device tensor as it is."""
    if isinstance(pairs, torch.Tensor):
        assert pairs.is_cuda and pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 4 and pairs.is_contiguous()
        return pairs
    if isinstance(pairs, ctypes.Array):
        host = np.frombuffer(pairs, dtype=np.uint32).reshape(-1, 4).copy() if len(pairs) else np.zeros((0, 4), dtype=np.uint32)
    else:
        host = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 4)
    return torch.from_numpy(host.view(np.int32)).to(dev)


def keygen_fixed_columns(chip, la: LookupArgument, kinds, k: int, blinding_factors: int, first_row: int = 0, layout=None, out=None):
    """(fixed, status): the NUM_FIXED fixed columns of an image's row kinds (h2r_keygen_fixed_columns), uint8 [15, 2^k, 32] in Lagrange form
    in the chip's representation: the image's rows from first_row on, the table's from row 0 on, 0 elsewhere.  kinds: uint8 row kinds
    (numpy or device tensor).  status: uint8 [1] on the device, H2R_E_SHAPE where a kind has no fixed row.  out: (fixed, status)."""
    dev = "cuda:%d" % chip.device
    n = 1 << int(k)
    kd = kinds_tensor(kinds, dev)
    fixed, status = outputs(out, dev, (torch.empty, torch.uint8, (NUM_FIXED, n, 32)), status=1)
    if not is_columns(fixed, rows=n, dims=(3,)) or fixed.shape[0] != NUM_FIXED:
        check(_lib.H2R_E_SHAPE, "keygen_fixed_columns")
    ws = workspace(lib().h2r_keygen_fixed_workspace_bytes(ctypes.byref(la.cfg)), dev)
    check(lib().h2r_keygen_fixed_columns(chip._ctx, ctypes.byref(la.cfg), ref(layout), kd.data_ptr(), kd.numel(), first_row, k, n - blinding_factors - 1,
                                         fixed.data_ptr(), fixed.stride(0), status.data_ptr(), ws.data_ptr(), chip._stream()), "h2r_keygen_fixed_columns")
    hold(chip, "keygen_fixed_columns", kd, ws, fixed, status)
    return fixed, status


def keygen_sigma_columns(chip, pairs, k: int, blinding_factors: int, delta: int, omega: int, column_src: Sequence[int] = (0, 1, 2, 3, 4),
                         first_row: int = 0, out=None):
    """(sigma, status, info): the sigma columns of a set of copy pairs (h2r_keygen_sigma_columns), uint8 [m, 2^k, 32] in the chip's
    representation: every class of cells ordered by (permutation column, row), sigma sends a cell to the label of its cyclic successor.
    pairs: see copy_pairs_tensor (rows counted from the image's first row; sources outside the image are dropped); delta, omega:
    integers in the chip's representation.  status: uint8 [1] on the device, H2R_E_SHAPE where a pair names a row >= 2^k -
    blinding_factors - 1 or a column that column_src does not hold.  info: hook_rounds, touched_cells, sort_passes.  out: (sigma, status)."""
    dev = "cuda:%d" % chip.device
    n, m = 1 << int(k), len(column_src)
    if not 0 < m <= _lib.H2R_PERM_MAX_COLUMNS:
        check(_lib.H2R_E_SHAPE, "keygen_sigma_columns")
    cd = copy_pairs_tensor(pairs, dev)
    cfg = _lib.H2RPermutationConfig(struct_size=ctypes.sizeof(_lib.H2RPermutationConfig), chunk_len=1)
    _permutation_columns(cfg, column_src)
    set_words(cfg.delta, delta)
    set_words(cfg.omega, omega)
    sigma, status = outputs(out, dev, (torch.empty, torch.uint8, (m, n, 32)), status=1)
    if not is_columns(sigma, rows=n, dims=(3,)) or sigma.shape[0] != m:
        check(_lib.H2R_E_SHAPE, "keygen_sigma_columns")
    ws = workspace(lib().h2r_keygen_sigma_workspace_bytes(k, m, cd.shape[0]), dev)
    info = _lib.H2RKeygenSigmaInfo(struct_size=ctypes.sizeof(_lib.H2RKeygenSigmaInfo))
    check(lib().h2r_keygen_sigma_columns(chip._ctx, ctypes.byref(cfg), cd.data_ptr() if cd.shape[0] else None, cd.shape[0], first_row, k,
                                         n - blinding_factors - 1, sigma.data_ptr(), sigma.stride(0), status.data_ptr(), ws.data_ptr(),
                                         ctypes.byref(info), chip._stream()), "h2r_keygen_sigma_columns")
    hold(chip, "keygen_sigma_columns", cd, ws, sigma, status)
    return sigma, status, info


def derive_vk_repr(vk: VerifyingKey, points: bytes) -> int:
    """This library's vk_repr of a verifying key (h2r_keygen_vk_repr): BLAKE2b-512, personalisation
    "H2R-VerifyKey-v1", over the configuration and the F + m + 1 key points (fixed, sigma, G: 64 bytes each, the chip's representation),
    reduced modulo r, in the chip's representation."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().h2r_keygen_vk_repr(vk.chip._ctx, ctypes.byref(vk.cfg), vk.dom.extended_k, bytes(points), out), "h2r_keygen_vk_repr")
    return from_words(out)


def keygen(chip, dom: EvaluationDomain, commit_key: CommitKey, la: LookupArgument, kinds, pairs, blinding_factors: int,
           column_src: Sequence[int] = (0, 1, 2, 3, 4), chunk_len: int = 2, first_row: int = 0, vk_repr: Optional[int] = None,
           lagrange_key: Optional[CommitKey] = None, layout=None) -> ProvingKey:
    """The ProvingKey of a circuit shape from what the library hands out (halo2's keygen_vk / keygen_pk): the row
    kinds (h2r_pow_row_kinds, fresh_op_row_kinds, ...), the copy pairs (chip.pow_copy_map; rows counted from the image's first row), the
    lookup configuration and a commit key.  The fixed and the sigma columns are built on the device, committed with the Lagrange key, and
    the F + m + 1 key points read back -- the call's one host trip besides the builders' own --; vk_repr is derived from them
    (derive_vk_repr) unless one is given (an integer in the chip's representation).  The constraint system is the one of an advice image:
    GATE_FIXED, LOOKUP_ADVICE / _TAG / _ENABLE, F_TABLE_TAG / _VALUE above, delta = field_delta(chip).  key.verifying_key() reuses the
    commitments formed here.  Raises H2RError(H2R_E_SHAPE) where a kind has no fixed row or a pair is refused."""
    k, n = dom.k, 1 << dom.k
    delta = field_delta(chip)
    fixed, st_fixed = keygen_fixed_columns(chip, la, kinds, k, blinding_factors, first_row=first_row, layout=layout)
    sigma, st_sigma, info = keygen_sigma_columns(chip, pairs, k, blinding_factors, delta, dom.omega, column_src, first_row=first_row)
    ck = commit_key if commit_key.n == n else CommitKey(chip, commit_key.bases[:n])
    lk = lagrange_key if lagrange_key is not None else dom.lagrange_key(ck)
    commitments = _key_commitments(lk, fixed, sigma)
    g = ck.bases[0].contiguous().view(torch.uint8).reshape(64)
    host = torch.cat([commitments[0].view(torch.uint8).reshape(-1), commitments[1].view(torch.uint8).reshape(-1), g, st_fixed, st_sigma]).cpu().numpy()
    for code in host[-2:]:
        check(int(code), "keygen")
    cfg = (blinding_factors, delta, GATE_FIXED, column_src, chunk_len, LOOKUP_ADVICE, LOOKUP_TAG, LOOKUP_ENABLE, F_TABLE_TAG, F_TABLE_VALUE)
    if vk_repr is None:
        vk_repr = derive_vk_repr(VerifyingKey(chip, dom, commitments[0], commitments[1], ck.bases[0], *cfg, 0), bytes(host[:-2]))
    key = ProvingKey(chip, dom, ck, la, fixed, sigma, kinds, *cfg, vk_repr, first_row=first_row, lagrange_key=lk)
    key.commitments, key.sigma_info = commitments, info
    return key


def msm_terms(chip, scalars: torch.Tensor, bases: torch.Tensor, num_terms: int, batch: int, scalars_stride: int, bases_stride: int, out: torch.Tensor,
              status: Optional[torch.Tensor] = None, scalars_off: int = 0, bases_off: int = 0) -> torch.Tensor:
    """out[e] = sum_{t < num_terms} s[e][t] * P[e][t] (h2r_msm_terms): uint8 [batch, 64] affine, (0, 0) for the identity.  Term t of circuit e:
    32 bytes at scalars + scalars_off + e * scalars_stride + 32 t, 64 bytes at bases + bases_off + e * bases_stride + 64 t (a stride of 0:
    one copy the batch shares); both in the chip's representation, any 256-bit scalar."""
    if (not 0 < num_terms <= _lib.H2R_VERIFY_MAX_TERMS or scalars.numel() * scalars.element_size() < scalars_off + (batch - 1) * scalars_stride + 32 * num_terms or
            bases.numel() * bases.element_size() < bases_off + (batch - 1) * bases_stride + 64 * num_terms or out.numel() * out.element_size() != 64 * batch):
        check(_lib.H2R_E_SHAPE, "msm_terms")      # (no assert: a short buffer must never reach the kernel)
    assert scalars.is_contiguous() and bases.is_contiguous() and out.is_contiguous()
    cfg = _lib.H2RMsmTermsConfig(struct_size=ctypes.sizeof(_lib.H2RMsmTermsConfig), num_terms=num_terms, reserved=0)
    check(lib().h2r_msm_terms(chip._ctx, ctypes.byref(cfg), scalars.data_ptr() + scalars_off, scalars_stride, bases.data_ptr() + bases_off, bases_stride,
                              batch, out.data_ptr(), ptr(status), chip._stream()), "h2r_msm_terms")
    return out


def verify_proof(vk: VerifyingKey, proofs: torch.Tensor, instances: Optional[torch.Tensor] = None, out=None):
    """(left, right, status): halo2's verify_proof (KZG, GWC) up to the pairing, for `batch` independent one-circuit proofs (DESIGN.md
    section 2n), with no host synchronisation.  proofs: uint8 [batch, vk.proof_bytes] on the device; instances: int64 [batch, I, 4],
    absorbed as common scalars.  left / right: uint8 [batch, 64], the affine accumulators L and R in the chip's representation: circuit e
    is ACCEPTED iff e(left[e], [tau]G2) = e(right[e], G2) -- the pairing is the caller's, once per batch over combine()'s fold.  status
    uint8 [batch]: H2R_E_SHAPE for a scalar >= r, an abscissa >= q or an instance that is not canonical, H2R_E_ASSERTION for an abscissa of
    no point or x^n = 1; a flagged circuit's left / right are left as they were (zeros when the call allocates).  out: (left, right,
    status) to write into; a status byte that is nonzero on entry skips the circuit; the call never clears it."""
    chip = vk.chip
    if proofs.dtype != torch.uint8 or proofs.dim() != 2 or proofs.shape[1] != vk.proof_bytes or proofs.shape[0] < 1 or not proofs.is_cuda:
        check(_lib.H2R_E_SHAPE, "verify_proof")
    assert proofs.is_contiguous()
    batch, dev, NB, NE = int(proofs.shape[0]), proofs.device, vk.num_bases, vk.num_evals
    left, right, status = outputs(out, dev, (torch.zeros, torch.uint8, (batch, 64)), (torch.zeros, torch.uint8, (batch, 64)), status=batch)
    # 1. decode: the proof's points at the head of every circuit's bases, the key's commitments and G behind them
    bases = torch.empty((batch, NB, 64), dtype=torch.uint8, device=dev)
    bases[:, vk.num_points:] = vk.key_bases
    evals = torch.empty((batch, NE, 32), dtype=torch.uint8, device=dev)
    sec = (_lib.H2RProofSection * len(vk.sections))()
    for d, (_, kind, count) in zip(sec, vk.sections):
        d.kind, d.count = _lib.H2R_TRANSCRIPT_POINT if kind == Transcript.POINT else _lib.H2R_TRANSCRIPT_SCALAR, count
    dcfg = _lib.H2RProofDecodeConfig(struct_size=ctypes.sizeof(_lib.H2RProofDecodeConfig), num_sections=len(vk.sections), reserved=0)
    check(lib().h2r_proof_decode(chip._ctx, ctypes.byref(dcfg), sec, proofs.data_ptr(), proofs.stride(0), batch, bases.data_ptr(), NB * 64,
                                 evals.data_ptr(), NE * 32, status.data_ptr(), chip._stream()), "h2r_proof_decode")
    # 2. the prover's rounds as common rounds, one more after the four W
    at, off = {}, 0
    for name, kind, count in vk.sections:
        if kind == Transcript.POINT:
            at[name] = (bases[:, off:off + count], Transcript.POINT)
            off += count
    tr = Transcript(chip, batch, 0)
    tr.round([(vk.vk, tr.SCALAR)] + ([(instances, tr.SCALAR)] if instances is not None and instances.shape[1] else []), common=True, status=status)

    def draw(names, squeeze):
        return tr.round([at[nm] for nm in names if nm in at], squeeze, common=True, status=status)[0]

    theta, bg = draw(["advice"], 1)[:, 0], draw(["lookup_perm"], 2)
    y, x = draw(["perm_z", "lookup_z", "random"], 1)[:, 0], draw(["h"], 1)[:, 0]
    v = tr.round([(evals, tr.SCALAR)], 1, common=True, status=status)[0][:, 0]
    u = draw(["w"], 1)[:, 0]
    # 3. the scalars of R (one per base) and of L (u^p over the four W)
    ch = _lib.H2RVerifyChallenges()
    held = [challenges(c, dev, batch) for c in (theta, bg[:, 0], bg[:, 1], y, x, v, u)]
    for name, c in zip(ch.NAMES, held):
        setattr(ch, name, c.data_ptr())
    rs = torch.empty((batch, NB, 32), dtype=torch.uint8, device=dev)
    ls = torch.empty((batch, 4, 32), dtype=torch.uint8, device=dev)
    check(lib().h2r_verify_scalars(chip._ctx, ctypes.byref(vk.cfg), evals.data_ptr(), NE * 32, ctypes.byref(ch), batch, rs.data_ptr(), NB * 32,
                                   ls.data_ptr(), status.data_ptr(), chip._stream()), "h2r_verify_scalars")
    # 4. R over all the bases, L over the four W where they lie among them
    msm_terms(chip, rs, bases, NB, batch, NB * 32, NB * 64, right, status)
    msm_terms(chip, ls, bases, 4, batch, 128, NB * 64, left, status, bases_off=vk.w_pos * 64)
    hold(vk, "verify_proof", proofs, instances, bases, evals, held, rs, ls, tr, left, right, status)
    return left, right, status


def combine(left: torch.Tensor, right: torch.Tensor, status: torch.Tensor, seed: bytes, chip):
    """(L*, R*), uint8 [64] each: the batch folded into ONE pair, L* = sum_e rho_e left[e] and R* = sum_e rho_e right[e], so that the
    caller's one pairing check e(L*, [tau]G2) = e(R*, G2) accepts every circuit whose status is 0 TOGETHER (a circuit with a nonzero
    status gets rho_e = 0 on the device and its points are not read: it is dropped, and stays rejected by its status).  That check runs on
    the device too: pairing_check(pkey, torch.stack((L*, R*))[None], 0b10) at batch 1.  rho_e is the
    generator's element (seed, circuit e, TAG_COMBINE, row 0) (h2r_random_columns).  `seed` (32 bytes) MUST BE UNKNOWN TO WHOEVER MADE THE
    PROOFS -- draw it after the proofs exist: one who knows rho can make two bad proofs whose errors cancel in the fold.  A batch above
    4,096 is summed in chunks of 4,096, and the chunks' sums once more."""
    batch, dev = int(left.shape[0]), left.device
    if len(seed) != 32 or batch < 1 or tuple(left.shape) != (batch, 64) or tuple(right.shape) != (batch, 64) or tuple(status.shape) != (batch,):
        check(_lib.H2R_E_SHAPE, "combine")
    rho = torch.zeros((batch, 1, 32), dtype=torch.uint8, device=dev)
    random_columns(chip, [rho], [TAG_COMBINE], (0, 1), seed)
    flagged = (status != 0)
    rho = torch.where(flagged[:, None, None], torch.zeros_like(rho), rho).reshape(batch, 32).contiguous()
    CH = _lib.H2R_VERIFY_MAX_TERMS
    chunks = (batch + CH - 1) // CH
    res = []
    for pts in (left, right):
        pts = torch.where(flagged[:, None], torch.zeros_like(pts), pts).contiguous()
        part = torch.zeros((chunks, 64), dtype=torch.uint8, device=dev)
        for c in range(chunks):
            n = min(CH, batch - c * CH)
            msm_terms(chip, rho, pts, n, 1, 0, 0, part[c], scalars_off=c * CH * 32, bases_off=c * CH * 64)
        if chunks > 1:
            wa, wb, one = ((ctypes.c_uint64 * 4)(*words(v)) for v in (1, 0, 1))       # 1 in the chip's representation
            if chip.montgomery:
                check(lib().h2r_field_eval(chip._ctx, _lib.FIELD_TO_MONTGOMERY, wa, wb, one), "h2r_field_eval")
            ones = torch.frombuffer(bytearray(from_words(one).to_bytes(32, "little") * chunks), dtype=torch.uint8).to(dev)
            part = msm_terms(chip, ones, part, chunks, 1, 0, 0, torch.zeros((1, 64), dtype=torch.uint8, device=dev))
        res.append(part.reshape(64))
    hold(chip, "combine", rho, res)
    return res[0], res[1]


# ---- the verdict: the pairing check ------------------------------------------------------------------------------------
class PairingKey:
    """The prepared tables of fixed G2 points, held on the device: h2r_pairing_prepare runs once per point on the host (102 line
    coefficients, 13,056 bytes per point), no G2 arithmetic runs per proof.  g2_points: up to 4 affine points of 128 bytes each (x.re, x.im,
    y.re, y.im in the chip's representation) as bytes or tensors.  The KZG verifier's key is PairingKey(chip, [tau_g2, g2]).  The points are
    key material: they must lie on the twist (checked) and in the subgroup of order r (NOT checked)."""

    def __init__(self, chip, g2_points):
        pts = [bytes(p.detach().cpu().contiguous().view(torch.uint8).reshape(-1).tolist()) if isinstance(p, torch.Tensor) else bytes(p) for p in g2_points]
        if not 0 < len(pts) <= _lib.H2R_PAIRING_MAX_PAIRS or any(len(p) != 128 for p in pts):
            check(_lib.H2R_E_SHAPE, "PairingKey")
        tabs = bytearray()
        for p in pts:
            t = (ctypes.c_uint8 * _lib.H2R_PAIRING_TABLE_BYTES)()
            check(lib().h2r_pairing_prepare(chip._ctx, p, t), "h2r_pairing_prepare")
            tabs += bytes(t)
        self.chip, self.num_pairs = chip, len(pts)
        self.tables = torch.frombuffer(tabs, dtype=torch.uint8).to("cuda:%d" % chip.device)


def pairing_check(pkey: PairingKey, points: torch.Tensor, negate_mask: int = 0, status: Optional[torch.Tensor] = None, out=None):
    """(accept, gt): for every circuit e the product over j of e(points[e][j], pkey's point j), y of pair j negated where bit j of
    negate_mask is set (h2r_pairing_products), with no host synchronisation.  points: uint8 [batch, num_pairs, 64] (or int64 [batch,
    num_pairs, 2, 4]) on the device, affine G1 points in the chip's representation, (0, 0) the identity; the rows of a circuit contiguous,
    any 16-byte-aligned stride between circuits.  accept uint8 [batch]: 1 iff the circuit's status is 0 after the call and the product is
    one, written for every circuit.  gt uint8 [batch, 384]: the product's value, left as it was for a flagged circuit (zeros when the call
    allocates).  status uint8 [batch]: nonzero on entry skips the circuit; H2R_E_SHAPE for a coordinate >= q, H2R_E_ASSERTION for a point
    off the curve; never cleared.  out: (accept, gt) to write into, either may be None to leave that output out."""
    chip, J = pkey.chip, pkey.num_pairs
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype not in (torch.uint8, torch.int64) or points.dim() < 2:
        check(_lib.H2R_E_SHAPE, "pairing_check")
    batch, row = int(points.shape[0]), points[0]
    if batch < 1 or row.numel() * row.element_size() != 64 * J or not row.is_contiguous():
        check(_lib.H2R_E_SHAPE, "pairing_check")
    stride = points.stride(0) * points.element_size() if batch > 1 else 64 * J
    accept, gt = outputs(out, points.device, (torch.empty, torch.uint8, (batch,)), (torch.zeros, torch.uint8, (batch, 384)))
    if (accept is not None and (accept.dtype != torch.uint8 or tuple(accept.shape) != (batch,))) or (gt is not None and (gt.dtype != torch.uint8 or tuple(gt.shape) != (batch, 384))):
        check(_lib.H2R_E_SHAPE, "pairing_check")
    assert (accept is None or accept.is_contiguous()) and (gt is None or gt.is_contiguous()) and (status is None or status.is_contiguous())
    cfg = _lib.H2RPairingConfig(struct_size=ctypes.sizeof(_lib.H2RPairingConfig), num_pairs=J, negate_mask=negate_mask, reserved=0)
    check(lib().h2r_pairing_products(chip._ctx, ctypes.byref(cfg), pkey.tables.data_ptr(), points.data_ptr(), stride, batch, ptr(gt), ptr(accept), ptr(status),
                                     chip._stream()), "h2r_pairing_products")
    hold(pkey, "pairing_check", points, status, accept, gt)
    return accept, gt


def verify(vk: VerifyingKey, pkey: PairingKey, proofs: torch.Tensor, instances: Optional[torch.Tensor] = None, out=None):
    """(accept, status): halo2's verify_proof to its verdict for `batch` independent one-circuit proofs, proof bytes in, no host access in
    between: verify_proof's accumulators, then e(left[e], [tau]G2) e(-right[e], G2) = 1 per circuit.  pkey: PairingKey(chip, [tau_g2, g2]).
    accept uint8 [batch]: 1 iff the circuit's status is 0 and the pairing check holds.  status as verify_proof's.  out: (accept, status) to
    write into; a status byte that is nonzero on entry skips the circuit."""
    batch, dev = int(proofs.shape[0]), proofs.device
    if pkey.num_pairs != 2:
        check(_lib.H2R_E_SHAPE, "verify")
    accept, status = outputs(out, dev, (torch.empty, torch.uint8, (batch,)), status=batch)
    acc = (torch.zeros((batch, 64), dtype=torch.uint8, device=dev), torch.zeros((batch, 64), dtype=torch.uint8, device=dev), status)
    left, right, _ = verify_proof(vk, proofs, instances, out=acc)
    pairing_check(pkey, torch.stack((left, right), dim=1), 0b10, status, out=(accept, None))
    return accept, status


# ---- KZG parameters from a known tau ---------------------------------------------------------------------------------
TAG_SETUP = 7 * 256                        # the generator's tag of setup's tau: kind 7, circuit 0, row 0


def _field(chip, op: int, a: int, b: int = 0) -> int:
    wa, wb, out = ((ctypes.c_uint64 * 4)(*words(v)) for v in (a, b, 0))
    check(lib().h2r_field_eval(chip._ctx, op, wa, wb, out), "h2r_field_eval")
    return from_words(out)


def field_omega(chip, k: int) -> int:
    """halo2's primitive 2^k-th root of unity of the chip's field (_lib.FIELD_ROOT_OF_UNITY squared down), in the chip's representation."""
    if chip.field not in _lib.FIELD_ROOT_OF_UNITY or not 0 < k <= _lib.FIELD_ROOT_OF_UNITY[chip.field][0]:
        check(_lib.H2R_E_SHAPE, "field_omega")
    s, w = _lib.FIELD_ROOT_OF_UNITY[chip.field]
    for _ in range(s - k):
        w = _field(chip, _lib.FIELD_MUL, w, w)
    return _field(chip, _lib.FIELD_TO_MONTGOMERY, w) if chip.montgomery else w


def curve_generator(chip) -> bytes:
    """The generator of the curve of the chip's field as a base: 64 bytes, x then y in the chip's representation."""
    if chip.field not in _lib.CURVE_GENERATOR:
        check(_lib.H2R_E_UNSUPPORTED, "curve_generator")
    q, xy = _lib.CURVE_GENERATOR[chip.field]
    return b"".join(((v << 256) % q if chip.montgomery else v).to_bytes(32, "little") for v in xy)


def fixed_base_table(chip, base: Optional[bytes] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [H2R_FIXED_BASE_TABLE_BYTES] on the device: T[w][d] = [d 256^w]B (h2r_fixed_base_table).  base: 64 host
    bytes, an affine point in the chip's representation ((0, 0): a table of identities); None: the curve's generator."""
    base = curve_generator(chip) if base is None else bytes(base)
    if len(base) != 64:
        check(_lib.H2R_E_SHAPE, "fixed_base_table")
    out = outputs(out, "cuda:%d" % chip.device, (torch.empty, torch.uint8, (_lib.H2R_FIXED_BASE_TABLE_BYTES,)))
    assert out.is_contiguous() and out.is_cuda and out.dtype == torch.uint8 and out.numel() == _lib.H2R_FIXED_BASE_TABLE_BYTES
    check(lib().h2r_fixed_base_table(chip._ctx, base, out.data_ptr(), chip._stream()), "h2r_fixed_base_table")
    return out


def fixed_base_mul(chip, table: torch.Tensor, scalars: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [n, 64]: out[i] = [scalars[i]]B for the base of `table` (h2r_fixed_base_mul): affine points in the chip's representation,
    (0, 0) the identity.  scalars: uint8 [n, 32] on the device, the chip's representation; out: the tensor to write into (it must overlap
    neither the scalars nor the table).  Never synchronises."""
    if not isinstance(scalars, torch.Tensor) or not scalars.is_cuda or not is_columns(scalars, dims=(2,), strides=False) or scalars.shape[0] == 0:
        check(_lib.H2R_E_SHAPE, "fixed_base_mul")
    assert is_columns(scalars) and table.is_cuda and table.is_contiguous() and table.numel() * table.element_size() == _lib.H2R_FIXED_BASE_TABLE_BYTES
    n = int(scalars.shape[0])
    out = outputs(out, scalars.device, (torch.empty, torch.uint8, (n, 64)))
    assert out.is_contiguous() and out.is_cuda and out.numel() * out.element_size() == 64 * n
    check(lib().h2r_fixed_base_mul(chip._ctx, table.data_ptr(), scalars.data_ptr(), n, out.data_ptr(), chip._stream()), "h2r_fixed_base_mul")
    hold(chip, "fixed_base_mul", table, scalars, out)
    return out


def setup_scalars(chip, mode: int, size: int, tau: int, omega: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [n, 32] on the device, the chip's representation (h2r_kzg_setup_scalars).  mode _lib.H2R_SETUP_POWERS: size = n, out[i] =
    tau^i; _lib.H2R_SETUP_LAGRANGE: size = k, n = 2^k, out[i] = l_i(tau) over the domain of omega (refused for a tau inside the domain).
    tau, omega: integers in the chip's representation."""
    lagrange, size = mode == _lib.H2R_SETUP_LAGRANGE, int(size)
    if mode not in (_lib.H2R_SETUP_POWERS, _lib.H2R_SETUP_LAGRANGE) or not 1 <= size <= (24 if lagrange else _lib.H2R_FIXED_BASE_MAX_POINTS):
        check(_lib.H2R_E_SHAPE, "setup_scalars")
    cfg =_lib.H2RSetupConfig(struct_size=ctypes.sizeof(_lib.H2RSetupConfig), mode=mode, log_n=size if lagrange else 0, reserved=0, n=0 if lagrange else size)
    set_words(cfg.tau, tau)
    set_words(cfg.omega, omega)
    n = (1 << size) if lagrange else size
    out = outputs(out, "cuda:%d" % chip.device, (torch.empty, torch.uint8, (n, 32)))
    assert out.is_contiguous() and out.is_cuda and out.numel() * out.element_size() == 32 * n
    check(lib().h2r_kzg_setup_scalars(chip._ctx, ctypes.byref(cfg), out.data_ptr(), chip._stream()), "h2r_kzg_setup_scalars")
    return out


def g2_generator(chip) -> bytes:
    """The generator of G2, 128 bytes in the chip's representation (h2r_g2_generator)."""
    out = (ctypes.c_uint8 * 128)()
    check(lib().h2r_g2_generator(chip._ctx, out), "h2r_g2_generator")
    return bytes(out)


def g2_mul(chip, g2: bytes, k: int) -> bytes:
    """[k]Q on the twist, on the host (h2r_g2_mul): g2 and the result are 128 bytes in the chip's representation, zeros the identity; k any
    integer below 2^256."""
    out = (ctypes.c_uint8 * 128)()
    check(lib().h2r_g2_mul(chip._ctx, bytes(g2), (ctypes.c_uint64 * 4)(*words(k)), out), "h2r_g2_mul")
    return bytes(out)


class Params:
    """halo2's ParamsKZG of a KNOWN tau (setup() below): k, n = 2^k, g = CommitKey over [tau^i]G, g_lagrange = CommitKey over [l_i(tau)]G,
    g2 and s_g2 = [tau]G2 as 128 host bytes.  keygen / ProvingKey take commit_key=params.g, lagrange_key=params.g_lagrange; verify takes
    params.pairing_key()."""

    def __init__(self, chip, k: int, omega: int, g: CommitKey, g_lagrange: CommitKey, g2: bytes, s_g2: bytes):
        self.chip, self.k, self.n, self.omega, self.g, self.g_lagrange, self.g2, self.s_g2 = chip, int(k), 1 << int(k), int(omega), g, g_lagrange, g2, s_g2

    def pairing_key(self) -> "PairingKey":
        """PairingKey(chip, [s_g2, g2]): what verify checks e(left, [tau]G2) e(-right, G2) = 1 against."""
        return PairingKey(self.chip, [self.s_g2, self.g2])

    def downsize(self, k2: int) -> "Params":
        """The parameters of the smaller domain 2^k2: the first 2^k2 points of g, g_lagrange by the curve transform over them
        (EvaluationDomain.lagrange_key) -- the powers of tau nest, the Lagrange basis does not."""
        if not 0 < k2 <= self.k:
            check(_lib.H2R_E_SHAPE, "Params.downsize")
        w = _field(self.chip, _lib.FIELD_FROM_MONTGOMERY, self.omega) if self.chip.montgomery else self.omega
        for _ in range(self.k - k2):
            w = _field(self.chip, _lib.FIELD_MUL, w, w)
        w = _field(self.chip, _lib.FIELD_TO_MONTGOMERY, w) if self.chip.montgomery else w
        g = CommitKey(self.chip, self.g.bases[:1 << k2])
        one = _field(self.chip, _lib.FIELD_TO_MONTGOMERY, 1) if self.chip.montgomery else 1
        return Params(self.chip, k2, w, g, EvaluationDomain(self.chip, k2, k2, w, one).lagrange_key(g), self.g2, self.s_g2)


def setup(chip, k: int, tau: Optional[int] = None, seed: Optional[bytes] = None, omega: Optional[int] = None) -> Params:
    """halo2's ParamsKZG::setup(k, rng) on the device: one fixed-base table of G, then the powers tau^i and the
    Lagrange values l_i(tau), each through h2r_fixed_base_mul, and [tau]G2 on the host.  No point array is copied to or from the host and
    nothing synchronises.
    A KNOWN TAU IS TOXIC WASTE: whoever holds it can open any commitment to any value.  This is for tests, benches and development keys, as
    the reference's setup is.  tau is not kept: the two scalar columns are zeroed on the stream once the multiplications have read them and
    the result references neither them nor the table; tau was in this process's host memory all the same.
    tau: an integer in the chip's representation; None: the generator's element (seed, circuit 0, TAG_SETUP, row 0) (h2r_random_eval),
    seed 32 bytes, os.urandom(32) when None.  A tau inside the domain (tau^n = 1) is refused (H2R_E_SHAPE).  omega: the primitive 2^k-th
    root of unity of the Lagrange basis (an EvaluationDomain's `omega`), in the chip's representation; None: field_omega(chip, k)."""
    k = int(k)
    if not 0 < k <= 24:
        check(_lib.H2R_E_SHAPE, "setup")
    if tau is None:
        seed = os.urandom(32) if seed is None else bytes(seed)
        if len(seed) != 32:
            check(_lib.H2R_E_SHAPE, "setup")
        out = (ctypes.c_uint64 * 4)()
        check(lib().h2r_random_eval(chip._ctx, seed, 0, TAG_SETUP, 0, out), "h2r_random_eval")
        tau = from_words(out)
    omega = field_omega(chip, k) if omega is None else int(omega)
    n = 1 << k
    lag = setup_scalars(chip, _lib.H2R_SETUP_LAGRANGE, k, tau, omega)     # (first: it refuses a tau inside the domain before anything is built)
    table = fixed_base_table(chip)
    pw = setup_scalars(chip, _lib.H2R_SETUP_POWERS, n, tau)
    g = CommitKey(chip, fixed_base_mul(chip, table, pw))
    g_lagrange = CommitKey(chip, fixed_base_mul(chip, table, lag))
    g2 = g2_generator(chip)
    s_g2 = g2_mul(chip, g2, _field(chip, _lib.FIELD_FROM_MONTGOMERY, tau) if chip.montgomery else tau)
    # the scalar columns are the toxic waste on the device (pw[1] is tau): cleared in stream order behind the multiplications that read
    # them, then released -- the launches run on torch's current stream, whose allocator reuses a block only behind them
    pw.zero_()
    lag.zero_()
    return Params(chip, k, omega, g, g_lagrange, g2, s_g2)
