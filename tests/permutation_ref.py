"""Plain model of halo2's permutation (copy-constraint) argument, Python big integers only [3P: plonk::permutation, restated in DESIGN.md
section 2e]: the evaluation domain's omega and delta, the sigma columns of a set of copy pairs (keygen's cycles), and the grand-product
columns Z of prover::commit by the literal recurrence.  The device's h2r_permutation_product_columns is compared with `product`."""

H2R_COPY_SRC = (0xFFFFFF01, 0xFFFFFF02, 0xFFFFFF03)   # h2r_copy.src_row of an operand outside the image (a, b, n)


def domain(P, k):
    """(omega, delta) as halo2's fields define them: with P - 1 = 2^S * t (t odd) and g a quadratic non-residue, the 2^S-th root of unity
    g^t brought down to exact order 2^k, and delta = g^(2^S) (a generator of the t-order subgroup: delta^c * omega^i are pairwise distinct)."""
    S, t = 0, P - 1
    while t % 2 == 0:
        S, t = S + 1, t // 2
    if k > S:
        raise ValueError("no domain of 2^%d rows: P - 1 = 2^%d * odd" % (k, S))
    g = 2
    while pow(g, (P - 1) // 2, P) != P - 1:     # Euler's criterion
        g += 1
    omega = pow(g, t << (S - k), P)
    return omega, pow(g, 1 << S, P)


def labels(m, u, delta, omega, P):
    """label_c(i) = delta^c * omega^i as [m][u]."""
    out, dc = [], 1
    for _ in range(m):
        col, x = [], dc
        for _ in range(u):
            col.append(x)
            x = x * omega % P
        out.append(col)
        dc = dc * delta % P
    return out


def sigma_from_pairs(pairs, m, u, delta, omega, P, column_of=None):
    """The sigma columns [m][u] of the copy pairs (row, col, src_row, src_col) over PHYSICAL image columns: union-find over the cells,
    every class ordered, sigma maps a cell to the label of the next cell of its cycle and is the identity elsewhere.  column_of: physical
    column -> permutation column (default: the identity).  Pairs whose source is an operand outside the image are dropped."""
    column_of = column_of or {c: c for c in range(m)}
    parent = {}

    def find(x):
        root = x
        while parent.setdefault(root, root) != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for (row, col, src_row, src_col) in pairs:
        if src_row in H2R_COPY_SRC:
            continue
        a, b = (column_of[col], row), (column_of[src_col], src_row)
        assert row < u and src_row < u
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    classes = {}
    for cell in list(parent):
        classes.setdefault(find(cell), []).append(cell)
    lab = labels(m, u, delta, omega, P)
    sigma = [list(col) for col in lab]
    for cells in classes.values():
        cells.sort()
        for i, (c, r) in enumerate(cells):
            nc, nr = cells[(i + 1) % len(cells)]
            sigma[c][r] = lab[nc][nr]
    return sigma


def columns(cells, extra, column_src, u, first_row=0):
    """v_c(i) as [m][u]: column_src[c] = 0..4 reads the PHYSICAL column of the image rows `cells` ([[5 integers]]) placed at first_row, 0 on
    every other usable row; 5 + j reads extra[j] (u integers)."""
    out = []
    for src in column_src:
        if src < 5:
            out.append([0] * first_row + [row[src] for row in cells] + [0] * (u - first_row - len(cells)))
        else:
            out.append(list(extra[src - 5][:u]))
        assert len(out[-1]) == u
    return out


def product(cells, extra, sigma, column_src, chunk_len, delta, omega, beta, gamma, u, P, first_row=0):
    """[S][u + 1]: Z_0[0] = 1, Z_s[0] = Z_{s-1}[u], Z_s[i+1] = Z_s[i] * n_s(i) / d_s(i); None from the first set on whose denominators
    hold a zero (the sets before it are returned).  The inversions of a set are batched (one pow per set)."""
    m = len(column_src)
    v = columns(cells, extra, column_src, u, first_row)
    lab = labels(m, u, delta, omega, P)
    out, start = [], 1
    for c0 in range(0, m, chunk_len):
        cs = range(c0, min(m, c0 + chunk_len))
        num, den = [1] * u, [1] * u
        for c in cs:
            vc, lc, sc = v[c], lab[c], sigma[c]
            for i in range(u):
                num[i] = num[i] * ((vc[i] + beta * lc[i] + gamma) % P) % P
                den[i] = den[i] * ((vc[i] + beta * sc[i] + gamma) % P) % P
        pre, acc = [], 1                      # batched inversion: prefix products, one inverse, walk back
        for x in den:
            pre.append(acc)
            acc = acc * x % P
        if acc == 0:
            return out + [None] * (len(range(c0, m, chunk_len)))
        inv_acc = pow(acc, -1, P)
        inv = [0] * u
        for i in range(u - 1, -1, -1):
            inv[i] = inv_acc * pre[i] % P
            inv_acc = inv_acc * den[i] % P
        z = [start]
        for i in range(u):
            z.append(z[-1] * num[i] % P * inv[i] % P)
        out.append(z)
        start = z[u]
    return out


def satisfying_cells(rng, m, u, n_cycles, P, max_len=5):
    """Synthetic columns [m][u] of random field elements made to satisfy random copy cycles; returns (v, pairs) with pairs as
    (row, col, src_row, src_col) over the m columns."""
    v = [[rng.randrange(P) for _ in range(u)] for _ in range(m)]
    cells = rng.sample(range(m * u), min(m * u, n_cycles * max_len))
    pairs, k = [], 0
    for _ in range(n_cycles):
        ln = rng.randrange(2, max_len + 1)
        cyc = cells[k:k + ln]
        k += ln
        if len(cyc) < 2:
            break
        c0, r0 = divmod(cyc[0], u)
        for x in cyc[1:]:
            c, r = divmod(x, u)
            v[c][r] = v[c0][r0]
            pairs.append((r, c, r0, c0))
    return v, pairs
