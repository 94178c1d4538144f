"""TEST HELPER: the copy constraints of the reference's RSA signature circuit outside the mul_mod records, by a plain walk of the
reference's control flow on cell ids.

Every main-gate / range-chip call ASSIGNS cells and returns the id (row, column) of the cell that holds its result; every call that
CONSUMES an id ties its input cell to that id: one pair (row, col, src_row, src_col).  The methods follow the reference method of the same
name line by line (file:line cited), as tests/circuit_rows.py does for the row counts; the cells of a call are the restated [3P]
main-gate shapes:

    assign_constant(v)        [v]                         result column 0
    assign_bit(v)             [v, v, v]                   result column 0
    add / sub / mul / and     [a, b, c]                   result column 2
    mul_add(a, b, c)          [a, b, c, a*b+c]            result column 3
    not(a)                    [a, 1-a]                    result column 1
    select(a, b, cond)        [cond, a, cond, b, out]     result column 4
    assert_equal(a, b)        [a, b]       assert_zero / assert_one(a)    [a]
    is_zero(a)                assign_bit(r); [a, a', r]; [r, a]           result: the bit
    is_equal(a, b)            sub(a, b), then is_zero of its result
    RangeChip::assign         two rows of sub-limbs (64-bit limb in 8-bit ones, 32-bit half in 4-bit ones); result column 4 of the first

Covered: assert_in_field (big_integer/chip.rs:1150-1158 and what it calls), the encoded-message check (src/chip.rs:137-198) and the
frame (benches/bench.rs:145-221).  The pow rows are skipped by their row count; `powed` is given as cells."""


class Walk:
    def __init__(self):
        self.n = 0            # next free row
        self.pairs = []       # (row, col, src_row, src_col)

    # ---- maingate / RangeChip [3P, restated shapes] -----------------------------------------------------------------------------
    def _row(self, *inputs):
        """one row; inputs[k] is the id consumed by column k (None: a cell the call assigns fresh)"""
        r = self.n
        self.n += 1
        for col, src in enumerate(inputs):
            if src is not None:
                self.pairs.append((r, col, src[0], src[1]))
        return r

    def assign_constant(self):
        return (self._row(), 0)

    def assign_bit(self):
        return (self._row(), 0)

    def add(self, a, b):
        return (self._row(a, b), 2)

    sub = mul = and_ = add

    def mul_add(self, a, b, c):
        return (self._row(a, b, c), 3)

    def not_(self, a):
        return (self._row(a), 1)

    def select(self, a, b, cond):
        return (self._row(cond, a, cond, b), 4)

    def assert_equal(self, a, b):
        self._row(a, b)

    def assert_zero(self, a):
        self._row(a)

    assert_one = assert_zero

    def is_zero(self, a):
        r = self.assign_bit()
        self._row(a, None, r)
        self._row(r, a)
        return r

    def is_equal(self, a, b):
        return self.is_zero(self.sub(a, b))

    def range_assign(self):
        r = self._row()
        self._row()
        return (r, 4)

    # ---- BigIntInstructions (big_integer/chip.rs) -----------------------------------------------------------------------------------
    def assign_integer(self, num_limbs):                                    # :62-82
        return [self.range_assign() for _ in range(num_limbs)]

    def max_value(self, num_limbs):                                         # :138-154
        return [self.assign_constant() for _ in range(num_limbs)]

    def add_int(self, a, b):                                                # :245-297
        max_n = max(len(a), len(b))
        zero_value = self.assign_constant()                                 # :259
        a = a + [zero_value] * (max_n - len(a))                             # :261
        b = b + [zero_value] * (max_n - len(b))                             # :263
        c_vals, carrys = [], [zero_value]                                   # :268
        limb_max_val = self.assign_constant()                               # :270
        for i in range(max_n):
            a_b = self.add(a[i], b[i])                                      # :272
            s = self.add(a_b, carrys[i])                                    # :273
            c = self.range_assign()                                         # :279-280
            carry = self.range_assign()                                     # :281-282
            c_add_carry = self.mul_add(carry, limb_max_val, c)              # :283
            self.assert_equal(s, c_add_carry)                               # :285
            c_vals.append(c)
            carrys.append(carry)
        c_vals.append(carrys[max_n])                                        # :290
        return c_vals

    def is_equal_fresh(self, a, b):                                         # :780-805
        n1, n2 = len(a), len(b)
        is_a_larger = n1 > n2
        eq_bit = self.assign_bit()                                          # :791
        for i in range(max(n1, n2)):
            if is_a_larger and i >= n2:
                flag = self.is_zero(a[i])                                   # :796
            elif not is_a_larger and i >= n1:
                flag = self.is_zero(b[i])                                   # :798
            else:
                flag = self.is_equal(a[i], b[i])                            # :800
            eq_bit = self.and_(eq_bit, flag)                                # :802
        return eq_bit

    def assert_equal_fresh(self, a, b):                                     # instructions.rs: is_equal_fresh + assert_one
        self.assert_one(self.is_equal_fresh(a, b))

    def sub_unchecked(self, a, b):                                          # :1286-1318
        assert len(a) >= len(b)
        c = [self.range_assign() for _ in range(len(a))]                    # :1304-1311
        added = self.add_int(b, c)                                          # :1315
        self.assert_equal_fresh(a, added)                                   # :1316
        return c

    def sub_int(self, a, b):                                                # :310-373
        n2 = len(b)
        max_int = self.max_value(n2)                                        # :319
        inflated_a = self.add_int(a, max_int)                               # :321
        inflated_subed = self.sub_unchecked(inflated_a, b)                  # :323
        one = self.assign_bit()                                             # :326
        is_not_overflowed = self.is_equal(inflated_subed[n2], one)          # :330
        is_overflowed = self.not_(is_not_overflowed)                        # :331
        num_limbs_l, num_limbs_r = len(inflated_subed), max(len(a), n2)
        zero_value = self.assign_constant()                                 # :339
        sel_l, sel_r = [], []
        for i in range(num_limbs_l):                                        # :345-357
            sel_l.append(self.select(inflated_subed[i], zero_value if i >= n2 else b[i], is_not_overflowed))
        for i in range(num_limbs_r):                                        # :358-367
            if i >= len(a):
                sel_r.append(self.select(max_int[i], zero_value, is_not_overflowed))
            elif i >= n2:
                sel_r.append(self.select(zero_value, a[i], is_not_overflowed))
            else:
                sel_r.append(self.select(max_int[i], a[i], is_not_overflowed))
        return self.sub_unchecked(sel_l, sel_r), is_overflowed              # :371

    def is_less_than(self, a, b):                                           # :908-919
        _, is_overflowed = self.sub_int(a, b)                               # is_less_than_or_equal :932-941
        is_eq = self.is_equal_fresh(a, b)
        is_not_eq = self.not_(is_eq)
        return self.and_(is_overflowed, is_not_eq)

    def assert_in_field(self, a, n):                                        # :1150-1158 (is_in_field = is_less_than :998-1006)
        self.assert_one(self.is_less_than(a, n))

    # ---- RSAChip (src/chip.rs) -------------------------------------------------------------------------------------------------------
    def encoded_message_check(self, is_eq, powed, hashed_msg):              # :139-198
        L = len(powed)
        for i in range(4):                                                  # :141-144
            is_eq = self.and_(is_eq, self.is_equal(powed[i], hashed_msg[i]))
        prefix_64_1 = self.assign_constant()                                # :149-152
        prefix_64_2 = self.assign_constant()
        e1 = self.is_equal(powed[4], prefix_64_1)                           # :153-154
        e2 = self.is_equal(powed[5], prefix_64_2)
        is_eq = self.and_(is_eq, e1)                                        # :155-156
        is_eq = self.and_(is_eq, e2)
        remain_low = self.range_assign()                                    # :170-171
        remain_high = self.range_assign()
        u32_assign = self.assign_constant()                                 # :172
        remain_concat = self.mul_add(remain_high, u32_assign, remain_low)   # :173
        self.assert_equal(powed[6], remain_concat)                          # :174
        prefix_32 = self.assign_constant()                                  # :175
        is_eq = self.and_(is_eq, self.is_equal(remain_low, prefix_32))      # :176-177
        ff_32 = self.assign_constant()                                      # :180
        is_eq = self.and_(is_eq, self.is_equal(remain_high, ff_32))         # :181-182
        ff_64 = self.assign_constant()                                      # :183-184
        for i in range(7, L - 1):                                           # :185-188
            is_eq = self.and_(is_eq, self.is_equal(powed[i], ff_64))
        last_em = self.assign_constant()                                    # :190-191
        return self.and_(is_eq, self.is_equal(powed[L - 1], last_em))       # :192-198


def in_field_pairs(L):
    """assert_in_field(a, n) alone, its operands named ("A", j) / ("B", j) as rows: the model of h2r_fresh_op_copy_map(IS_IN_FIELD | ASSERT_ONE)."""
    w = Walk()
    w.assert_in_field([("A", j) for j in range(L)], [("B", j) for j in range(L)])
    return w.n, w.pairs


def signature_circuit(L, pow_rows, record_rows, num_mul_mods):
    """The Fix-exponent signature circuit (benches/bench.rs:145-221): returns (rows, pairs outside the pow rows, first pow row, cells)
    with cells = dict of the sig / n / hashed ids.  pow_rows: rows of pow_mod_fixed_exp's section (CONST1, CONST0, then num_mul_mods
    records of record_rows rows); powed = the r limbs of the last record (limb j: column e of the first row of its RangeChip::assign,
    the (L + j)-th of the record)."""
    w = Walk()
    sig = w.assign_integer(L)                                               # assign_signature :150
    n = w.assign_integer(L)                                                 # assign_public_key :151-152 (Fix: e assigns nothing)
    hashed = w.assign_integer(4)                                            # :201-202
    is_eq = w.assign_constant()                                             # src/chip.rs:137
    w.assert_in_field(sig, n)                                               # modpow_public_key :106
    pow_first = w.n
    w.n += pow_rows                                                         # pow_mod_fixed_exp :111 (h2r_pow_copy_map's rows)
    last = pow_first + 2 + (num_mul_mods - 1) * record_rows
    powed = [(last + 2 * (L + j), 4) for j in range(L)]
    is_valid = w.encoded_message_check(is_eq, powed, hashed)
    w.assert_one(is_valid)                                                  # benches/bench.rs:218
    return w.n, w.pairs, pow_first, dict(sig=sig, n=n, hashed=hashed)
