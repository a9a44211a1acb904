"""What the tests of the direct CIC / TSC deposit (vps_deposit_assign) share: a numpy restatement of the record's six weight
words and of the weights the accumulation kernel forms from them (the same expressions, the same float32 rounding points), the
half-cell lattice on which every sum is exact in float32 in any order, and the count of non-zero contributions per cell.

TEST INFRASTRUCTURE ONLY; tests/test_assign_direct_cpu.py pins the first two to tests/small_ref.py."""
import numpy as np

import small_ref as sr

LCELL = 2.0 ** -7            # cell length of the lattice cases: L = N / 128, positions are multiples of LCELL / 2


def record_words(pos, N, L, assignment):
    """float32 [np, 3, 2]: per axis the two numbers a record carries, each rounded ONCE from float64.
    CIC: (1 - f, f), the weights themselves.  TSC: a = 1/2 - d, b = 1/2 + d."""
    s = np.asarray(pos, dtype=np.float64) / (L / float(N))
    if sr.ORDER[assignment] == 2:
        f = s - 0.5 - np.floor(s - 0.5)
        return np.stack((1.0 - f, f), axis=-1).astype(np.float32)
    d = s - (np.floor(s) + 0.5)
    return np.stack((0.5 - d, 0.5 + d), axis=-1).astype(np.float32)


def weights_from_words(words, assignment):
    """float32 [np, 3, order]: what the accumulation kernel makes of the words, in float32 arithmetic (every numpy float32
    operation rounds once, as the kernel's does without contraction)."""
    a, b = words[..., 0], words[..., 1]
    assert a.dtype == np.float32 and b.dtype == np.float32
    if sr.ORDER[assignment] == 2:
        return np.stack((a, b), axis=-1)
    h = np.float32(0.5)
    return np.stack((h * (a * a), h + a * b, h * (b * b)), axis=-1)


def lattice_particles(N, assignment, bricks, C, seed, n_random=20000, copies=3):
    """(pos float64 [n, 3], f float32 [n, C]) on the half-cell lattice: positions are integer multiples of LCELL / 2 (exact in
    float32 and float64, inside the box and up to two box lengths outside it), payloads integers in [-8, 8].  Every CIC weight
    is then 1, 0 or 1/2 and every TSC weight 1/2, 0, 1/8 or 3/4: products are multiples of 2^-9 and a cell's sum of a few
    hundred of them is exact in float32 in any order.
      - a regular sub-lattice whose particles together touch EVERY cell of the grid: CIC particles on the faces between cells
        c and c + 1 for every second c per axis (weights 1/2, 1/2), TSC particles on the centre of every third cell (weights
        1/8, 3/4, 1/8);
      - for every axis and every brick of `bricks` = (bx, by, bz) its first and its last cell, aimed at from every offset
        j < order with both half-cell parities (particles whose base cell is that cell minus j), the other two coordinates
        random;
      - n_random particles anywhere on the lattice from -N to 2 N cells."""
    order = sr.ORDER[assignment]
    rng = np.random.default_rng(seed)
    L = N * LCELL
    if order == 2:
        h1 = 2 * np.arange(0, N, 2) + 2              # s = c + 1: on the face, base cell c
    else:
        h1 = 2 * np.arange(1, N + 1, 3) + 1          # s = c + 1/2: on the centre of c, base cell c - 1
    cover = np.stack(np.meshgrid(h1, h1, h1, indexing="ij"), axis=-1).reshape(-1, 3)
    parts = [cover, rng.integers(-2 * N, 4 * N, (n_random, 3))]
    for a, bw in enumerate(bricks):
        firsts = np.arange(0, N, bw)
        edge_cells = np.unique(np.concatenate((firsts, np.minimum(firsts + bw, N) - 1)))
        for j in range(order):
            for parity in (0, 1):
                c0 = edge_cells - j                   # base cell; half-steps of a position with that base cell:
                h = 2 * c0 + (1 + parity if order == 2 else 2 + parity)     # CIC s in [c0 + 1/2, c0 + 3/2), TSC s in [c0 + 1, c0 + 2)
                for _ in range(copies):
                    p = rng.integers(0, 2 * N, (len(h), 3))
                    p[:, a] = h
                    parts.append(p)
    h = np.concatenate(parts).astype(np.int64)
    pos = h * (LCELL / 2)
    f = rng.integers(-8, 9, (len(pos), C)).astype(np.float32)
    assert np.abs(h).max() < 2 ** 23
    return pos, f, L


def contribution_counts(pos, N, L, assignment):
    """(cells sorted [m], n [m]): per flat cell the number of (particle, offset) pairs with a non-zero weight product."""
    order = sr.ORDER[assignment]
    c0, w = sr.assign_weights(pos, N, L, assignment)
    dense = N ** 3 <= 1 << 25
    flats, count = [], np.zeros(N ** 3 if dense else 0, dtype=np.int64)
    for jx in range(order):
        for jy in range(order):
            for jz in range(order):
                wt = w[:, 0, jx] * w[:, 1, jy] * w[:, 2, jz]
                flat = (((c0[:, 0] + jx) % N) * N + (c0[:, 1] + jy) % N) * N + (c0[:, 2] + jz) % N
                if dense:
                    count += np.bincount(flat[wt != 0], minlength=N ** 3)
                else:
                    flats.append(flat[wt != 0])
    if dense:
        cells = np.flatnonzero(count)
        return cells, count[cells]
    return np.unique(np.concatenate(flats), return_counts=True)
