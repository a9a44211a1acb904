"""Per-cell parity of the gridding -- bucket sort, brick accumulate, fused pencil deposit + z pass -- at the sort geometries
the production sizes select, against references that are exact at any size (oracle/gpu_checks.py; pinned to the oracle by
tests/test_gridding_reference_cpu.py).

The particles are CONSTRUCTED: integer cells first, positions strictly inside them, rho in 1..3 and v in -3..3, no cell total
above 2^12.  NGP sums of such payloads are exact in float32, so the right answer of a raw deposit is an int64 histogram, and
the momentum launch of the fused route (vol * sum rho v_c, no division) must give those integers back when its z image is
inverted in float64.  Every leg first asserts, through K.deposit_plan, the sort path it is there to exercise.  Legs:
  a. coverage guard: every plan value of the list occurs in the matrix, and the plans of the bench configurations (C2, C4, the
     C5 rank share, the brick deposits of deposit_to_grid at 1024 / 2048) are among those exercised;
  b. vps_deposit_ngp bit for bit, slab by slab over the whole grid, 48^3 ... 2048^3 with 1, 3 and 4 channels;
  c. vps_deposit_field: mass and momentum exact on integer data, v / E and every field of lognormal data per cell against float64;
  d. vps_deposit_fft_z[_slab]: the inverted z images round to the exact integers in every cell, at most INT_DIST away;
  e. b and d at 2048 under sort_atomic = 1, sort_staged = 0 and sort_groups = 4096;
  f. (last) what the legs actually ran covers what leg a counted.
Plan flags = every plan field except nchunks and cap_in (the two that only count particles)."""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import gpu_checks as chk  # noqa: E402

V_RTOL, V_ATOL = 2e-5, 1e-6   # v per cell (test_float64_positions_through_fused_deposit); m: V_RTOL alone; empty cells exactly 0
E_RTOL = 1e-4                 # E per cell (same test)
FIELD_ATOL = 1e-5             # inverted z images of v, E, w: max error / rms of the field (the thin-slab tests' bar)
INT_DIST = 0.25               # inverted momentum images: largest distance from an integer

# (N, C, particles) of the raw brick deposits; the first entry of a size is the one that runs every distribution
BRICKS = ((512, 4, 10_000_000), (1024, 3, 50_000_000), (1024, 1, 50_000_000), (1024, 4, 50_000_000), (2048, 1, 100_000_000),
          (2048, 4, 100_000_000), (2048, 3, 100_000_000), (96, 3, 1_000_000), (250, 1, 4_000_000), (384, 4, 8_000_000),
          (48, 4, 1_000_000))
# (N, particles) of the whole-grid pencil deposits
PENCILS = ((512, 10_000_000), (1024, 50_000_000), (2048, 100_000_000), (384, 8_000_000), (768, 30_000_000), (250, 4_000_000),
           (500, 10_000_000))
C5_SHARE = (4096, 1536, 512, 1_000_000_000)       # N, x0, nx, replicated particles: one rank's share of C5
FLAVOURS = ({"sort_atomic": 1}, {"sort_staged": 0}, {"sort_groups": 4096})
FLAG_FIELDS = ("bx", "by", "bz", "nbuckets", "cells", "cells_pow2", "two_level", "wide_keys", "gshift", "ngroups", "staged",
               "staged_lds", "recompute")


@pytest.fixture(scope="module")
def K():
    from vpower import device
    yield device.default_kernels()


@pytest.fixture(autouse=True)
def _peak_memory_of_the_leg(request):
    """Prints the device-memory high-water mark of every leg above 100 GB (the docstrings state what each needs)."""
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated() / 1e9
    if peak > 100:
        print("\n%s: peak device memory %.1f GB" % (request.node.name, peak))


def _free(K):
    K._work.clear()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _options(opts):
    """Library options for the duration of the block; restored in a finally."""
    from vpower import _ffi
    prev = {k: _ffi.OPTIONS.get(k) for k in opts}
    try:
        for k, v in opts.items():
            _ffi.set_option(k, v)
        yield
    finally:
        for k, v in prev.items():
            _ffi.set_option(k, v)


RAN = []     # what every leg actually ran: its plan + C, position dtype and a name (test_f reads it)


def _ran(plan, name, C, pos):
    RAN.append(dict(plan, name=name, C=C, dtype=str(pos.dtype).replace("torch.", "")))


def _flags(plan):
    return tuple(plan[f] for f in FLAG_FIELDS)


def _expect(plan, **want):
    got = {k: plan[k] for k in want}
    assert got == want, (got, want, plan)


def _bucket(plan, N, x0, x, y, z):
    nby, nbz = -(-N // plan["by"]), -(-N // plan["bz"])
    return (((x - x0) // plan["bx"]) * nby + y // plan["by"]) * nbz + z // plan["bz"]


def _assert_equal_cells(got, want, N, x0, plan, what):
    """got, want: flat tensors over the rows from x0 on, cell (x, y, z) at ((x - x0) N + y) N + z.  A mismatch names the first
    offending cells: index, got, want, bucket."""
    bad = torch.nonzero(got != want).squeeze(1)
    if bad.numel():
        first = []
        for i in bad[:6].tolist():
            x, y, z = x0 + i // (N * N), (i // N) % N, i % N
            first.append("cell (%d, %d, %d): got %r, want %r, bucket %d" % (x, y, z, got[i].item(), want[i].item(),
                                                                           _bucket(plan, N, plan.get("x0", 0), x, y, z)))
        raise AssertionError("%s: %d cells differ; %s" % (what, bad.numel(), "; ".join(first)))


def _particles(K, n, N, dist, seed, dtype=None):
    L, dt = chk.matrix_geometry(N, dtype)
    if dist == "ends":
        n = chk.ends_count(n)
    return (L,) + chk.constructed_particles(K.device, n, N, L, dt, dist, seed=seed)


def _rows(N, nx, budget=1 << 28):
    return max(1, min(nx, budget // (N * N)))


def _int_payload(rho, vel, C):
    r = rho.to(torch.int64)
    if C == 1:
        return r[:, None].contiguous()
    rv = r[:, None] * vel.to(torch.int64)
    return rv if C == 3 else torch.cat([rv, r[:, None]], dim=1)


# ------------------------------------------------------------------------------------------- a ----
def _matrix_plans(K):
    """{leg name: plan} of every leg below, under the options the leg runs with."""
    plans = {}
    for N, C, n in BRICKS:
        plans["brick %d C=%d" % (N, C)] = K.deposit_plan(n, C, N, 0, N)
        plans["field %d" % N] = K.deposit_plan(n, 4, N, 0, N)
    for N, n in PENCILS:
        if K.fused_supported(N, 1):
            plans["pencil %d" % N] = K.deposit_plan(n, 4, N, 0, N, pencil=True)
    plans["pencil 2048 rows 512..1535"] = K.deposit_plan(PENCILS[2][1], 4, 2048, 512, 1024, pencil=True)
    N, x0, nx, n = C5_SHARE
    plans["pencil 4096 slab"] = K.deposit_plan(n, 4, N, x0, nx, pencil=True, slab_particles=n // 8)
    plans["pencil 4096 plain"] = K.deposit_plan(n, 4, N, x0, nx, pencil=True)
    for opts in FLAVOURS:
        with _options(opts):
            plans["brick 2048 C=1 %r" % (opts,)] = K.deposit_plan(100_000_000, 1, 2048, 0, 2048)
            plans["pencil 2048 %r" % (opts,)] = K.deposit_plan(100_000_000, 4, 2048, 0, 2048, pencil=True)
    return plans


def test_a_coverage_guard(K):
    """Every sort path of the list is in the matrix (the >64 KiB staged scatter through sort_groups = 4096 on the 2048 pencils: no
    natural geometry has the 2041 groups it takes), and so are the plans of the bench configurations.  The automatic
    two_level = 0 fallback needs more than 2^23 buckets -- 2^35 cells of bricks, or 16384 rows of 4096-point pencils -- which no
    grid of one card has: it is not in the matrix."""
    plans = _matrix_plans(K)
    for name, p in plans.items():
        print(name, {k: p[k] for k in FLAG_FIELDS + ("nchunks", "cap_in")})
    vals = list(plans.values())

    def some(**want):
        return any(all(p[k] == v for k, v in want.items()) for p in vals)

    assert some(wide_keys=0) and some(wide_keys=1)
    assert some(two_level=1) and plans["brick 2048 C=1 %r" % (FLAVOURS[0],)]["two_level"] == 0
    assert any(p["staged"] == 1 and p["staged_lds"] <= 64 * 1024 for p in vals)
    assert any(p["staged"] == 1 and p["staged_lds"] > 64 * 1024 for p in vals)
    assert any(p["two_level"] == 1 and p["staged"] == 0 for p in vals)
    assert some(gshift=3) and some(gshift=12) and any(3 < p["gshift"] < 12 for p in vals)
    assert some(recompute=0) and some(recompute=1)
    assert some(cells_pow2=1) and some(cells_pow2=0)
    assert {C for _, C, _ in BRICKS} == {1, 3, 4}
    assert {dt for _, _, dt in chk.GRIDDING_MATRIX} == {"float32", "float64"}
    assert any(p["bz"] == 2048 and p["bx"] == 1 for p in vals) and any(p["bz"] == 64 for p in vals)      # pencils and bricks
    exercised = {_flags(p) for p in vals}
    bench = {"C2": K.deposit_plan(10_000_000, 4, 512, 0, 512, pencil=True),
             "C4": K.deposit_plan(100_000_000, 4, 2048, 0, 2048, pencil=True),
             "C5 share": K.deposit_plan(1_000_000_000, 4, 4096, 3584, 512, pencil=True, slab_particles=125_000_000)}
    for N, n in ((1024, 50_000_000), (2048, 100_000_000)):
        for C in (1, 3, 4):
            bench["deposit_to_grid %d C=%d" % (N, C)] = K.deposit_plan(n, C, N, 0, N)
    for name, p in bench.items():
        assert _flags(p) in exercised, (name, p)


# ------------------------------------------------------------------------------------------- b ----
def _check_raw_deposit(K, N, C, n, dist, seed, dtype=None, slab=None, **expect):
    L, cells, pos, rho, vel = _particles(K, n, N, dist, seed, dtype)
    plan = K.deposit_plan(pos.shape[0], C, N, 0, N)
    _expect(plan, **expect)
    _ran(plan, "brick %d C=%d" % (N, C), C, pos)
    pay = _int_payload(rho, vel, C)
    fpay = pay.float().contiguous()
    grid = K.deposit(pos, fpay, N, L, 0, N)                    # [C, N, N, N]
    rows = _rows(N, N)
    for x0 in range(0, N, rows):
        r = min(rows, N - x0)
        want = chk.exact_slab_reference(cells, None, None, N, x0, r, payload=pay)
        for c in range(C):
            assert int(want[c].abs().max()) <= chk.CELL_SUM_CAP
            _assert_equal_cells(grid[c, x0:x0 + r].reshape(-1), want[c].float(), N, x0, plan,
                                "deposit %d^3 C=%d %s channel %d" % (N, C, dist, c))
        del want
    if slab is not None:                                       # a slab x0 > 0: the same rows of the whole-grid result
        x0, nx = slab
        part = K.deposit(pos, fpay, N, L, x0, nx)
        assert torch.equal(part, grid[:, x0:x0 + nx]), "slab [%d, %d) differs from the whole grid's rows" % (x0, x0 + nx)
    del grid
    _free(K)


@pytest.mark.parametrize("dist", chk.DISTRIBUTIONS)
def test_b_deposit_512(K, dist):
    """512^3, C = 4, 1e7 particles (2.1 GB of output)."""
    _check_raw_deposit(K, 512, 4, 10_000_000, dist, 11, wide_keys=0, two_level=1, staged=1, cells_pow2=1)


def test_b_deposit_512_float64_positions(K):
    _check_raw_deposit(K, 512, 4, 10_000_000, "clump", 12, dtype="float64", wide_keys=0, two_level=1)


@pytest.mark.parametrize("C,dist", [(3, "uniform"), (3, "clump"), (1, "uniform"), (4, "uniform")])
def test_b_deposit_1024(K, C, dist):
    """1024^3, 5e7 particles with float64 positions (C = 4: 17 GB of output)."""
    _check_raw_deposit(K, 1024, C, 50_000_000, dist, 13, wide_keys=0, two_level=1, staged=1)


@pytest.mark.parametrize("dist", chk.DISTRIBUTIONS)
def test_b_deposit_2048_one_channel(K, dist):
    """2048^3, C = 1, 1e8 particles, 64-bit keys.  34 GB of output + 2 GB of particles + 3 GB of workspace + 5 GB of reference."""
    _check_raw_deposit(K, 2048, 1, 100_000_000, dist, 14, slab=(1000, 40) if dist == "uniform" else None,
                       wide_keys=1, two_level=1, staged=1)


@pytest.mark.parametrize("C,dist", [(4, "uniform"), (4, "clump"), (3, "uniform")])
def test_b_deposit_2048(K, C, dist):
    """2048^3, 1e8 particles; C = 4 is the geometry of vps_deposit_field: gshift at its clamp of 12.  137 GB of output (C = 3: 103)
    + 5 GB of particles and integer payload + 6 GB of workspace + 9 GB of reference slabs."""
    want = dict(gshift=12, ngroups=512) if C == 4 else {}
    _check_raw_deposit(K, 2048, C, 100_000_000, dist, 15, wide_keys=1, two_level=1, staged=1, **want)


@pytest.mark.parametrize("N,C,n,expect", [(96, 3, 1_000_000, dict(gshift=3, cells_pow2=1)), (250, 1, 4_000_000, {}),
                                          (384, 4, 8_000_000, {}), (48, 4, 1_000_000, dict(cells_pow2=0, gshift=3))])
@pytest.mark.parametrize("dist", ["uniform", "clump"])
def test_b_deposit_ragged(K, N, C, n, expect, dist):
    """Whole grids whose bricks have a ragged edge (96, 250, 384) and, at 48, a cell count that is not a power of two."""
    _check_raw_deposit(K, N, C, n, dist, 16, wide_keys=0, **expect)


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 100_003])
def test_b_deposit_particle_count_edges(K, n):
    """Around one level-1 chunk (SORT_CHUNK = 2048 particles) and a count that is no multiple of 256, at 96^3."""
    plan = K.deposit_plan(n, 1, 96, 0, 96)
    assert plan["nchunks"] == -(-n // 2048)
    _check_raw_deposit(K, 96, 1, n, "uniform", 17 + n, two_level=1)


# ------------------------------------------------------------------------------------------- c ----
def _ratio(got, ref, tol):
    """max |got - ref| / tol over the cells (tol > 0 everywhere it matters; 0 / 0 counts as 0)."""
    d = (got.double() - ref).abs()
    return float(torch.where(d > 0, d / tol, torch.zeros_like(d)).max())


def _check_field(K, N, n, dist, seed, integer, quantities):
    """vps_deposit_field against the float64 fields of the same cell totals, one quantity at a time, slab by slab.  Bars per cell:
    v: V_RTOL |v| + V_ATOL; m: V_RTOL m; p = v m: V_RTOL |p| + V_ATOL m (v's absolute term times the cell's mass);
    E = m |v|^2: E_RTOL E + 2 V_ATOL m (|vx| + |vy| + |vz|) (the first-order effect of v's absolute term); a cell without
    particles is exactly 0 in every field.  Integer data with L = 1, N = 2^k: m and p bit for bit.  -> worst ratio per field."""
    from vpower import device
    L, cells, pos, rho, vel = _particles(K, n, N, dist, seed)
    if not integer:
        g = torch.Generator(device=K.device)
        g.manual_seed(seed)
        rho = torch.exp(0.5 * torch.randn(rho.shape, generator=g, device=K.device))
        vel = torch.randn(vel.shape, generator=g, device=K.device)
    plan = K.deposit_plan(pos.shape[0], 4, N, 0, N)
    _expect(plan, two_level=1, wide_keys=int(N == 2048))
    _ran(plan, "field %d" % N, 4, pos)
    vol = (L / N) ** 3
    exact = integer and L == 1.0 and N & (N - 1) == 0
    rows = _rows(N, N, 1 << 26)                                # (a dozen float64 reference fields per block of rows)
    worst = {}
    for q in quantities:
        out = K.deposit_field(pos, vel, rho, N, L, 0, N, device.VM if q == "vm" else device.QUANTITY[q])
        for x0 in range(0, N, rows):
            r = min(rows, N - x0)
            if integer:
                s = chk.exact_slab_reference(cells, rho, vel, N, x0, r)
                f = chk.ngp_fields_float64(s[0].double(), [a.double() for a in s[1:]], vol, ("velocity", "mass", "momentum", "energy"))
            else:
                f = chk.float64_slab_fields(cells, rho, vel, N, L, x0, r, ("velocity", "mass", "momentum", "energy"))
            m = f["mass"][0]
            empty = m == 0
            got = [out[c, x0:x0 + r].reshape(-1) for c in range(out.shape[0])]
            for c, gc in enumerate(got):
                assert not bool((gc[empty] != 0).any()), "%s %d^3: channel %d of an empty cell is not 0" % (q, N, c)
            absv = f["velocity"][0].abs() + f["velocity"][1].abs() + f["velocity"][2].abs()
            if q in ("vm", "velocity"):
                for c in range(3):
                    ref = f["velocity"][c]
                    worst["v"] = max(worst.get("v", 0.0), _ratio(got[c], ref, V_RTOL * ref.abs() + V_ATOL))
                if q == "vm":
                    if exact:
                        _assert_equal_cells(got[3], m.float(), N, x0, plan, "deposit_field %d^3 %s mass" % (N, dist))
                    worst["m"] = max(worst.get("m", 0.0), _ratio(got[3], m, V_RTOL * m))
            elif q == "momentum":
                for c in range(3):
                    ref = f["momentum"][c]
                    if exact:
                        _assert_equal_cells(got[c], (s[1 + c].double() * vol).float(), N, x0, plan,
                                            "deposit_field %d^3 %s momentum %d" % (N, dist, c))
                    worst["p"] = max(worst.get("p", 0.0), _ratio(got[c], ref, V_RTOL * ref.abs() + V_ATOL * m))
            else:
                ref = f["energy"][0]
                worst["E"] = max(worst.get("E", 0.0), _ratio(got[0], ref, E_RTOL * ref + 2 * V_ATOL * m * absv))
            del f, got, m, empty, absv
        del out
        _free(K)
    print("deposit_field %d^3 %s %s: worst |got - ref| / bar per field %s"
          % (N, dist, "integer" if integer else "lognormal", {k: "%.3g" % v for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst
    return worst


# (N, particles) of the vps_deposit_field legs: the sizes of b
FIELD_SIZES = ((512, 10_000_000), (1024, 50_000_000), (2048, 100_000_000), (96, 1_000_000), (250, 4_000_000), (384, 8_000_000))


@pytest.mark.parametrize("N,n", FIELD_SIZES)
@pytest.mark.parametrize("dist", ["uniform", "clump"])
def test_c_deposit_field_integer_data(K, N, n, dist):
    """Every size of b with both distributions: v and E within the per-cell bar; mass and momentum bit exact where L = 1 and
    N = 2^k (512, 1024, 2048).  2048: 137 GB of output (VM) + 3 GB of particles + 6 GB of workspace + 40 GB of int64 and float64
    reference slabs."""
    _check_field(K, N, n, dist, 21, True, ("vm", "momentum", "energy"))


@pytest.mark.parametrize("N,n", FIELD_SIZES)
@pytest.mark.parametrize("dist", ["uniform", "clump"])
def test_c_deposit_field_lognormal_data(K, N, n, dist):
    """Real-valued rho = exp(N(0, 0.25)), v = N(0, 1) at constructed positions, every size of b with both distributions; memory
    as for the integer data.  (The velocity quantity is the v of VM without the mass channel: launched below 2048 only.)"""
    qs = ("vm", "velocity", "momentum", "energy") if N < 2048 else ("vm", "momentum", "energy")
    _check_field(K, N, n, dist, 22, False, qs)


# ------------------------------------------------------------------------------------------- d ----
def _invert_rows(img, N, nx, i, j):
    """Rows [i, j) of the real field behind one z image (flat complex64: B[x][kz][y] for kz < N/2, then the Nyquist plane
    BN[x][y]): complex128 inverse real transform along kz -> float64 [j - i, y, z]."""
    h = N // 2
    B = img[: nx * h * N].view(nx, h, N)[i:j].to(torch.complex128)
    BN = img[nx * h * N:].view(nx, 1, N)[i:j].to(torch.complex128)
    return torch.fft.irfft(torch.cat([B, BN], dim=1), n=N, dim=1).transpose(1, 2)


def _check_images(K, N, L, x0, nx, cells, rho, vel, plan, what, integer=(), real=()):
    """integer: [(z image, channel c)]: image / vol must round to the exact sum rho v_c in every cell, at most INT_DIST away.
    real: [(z image, name, field key, component, scale)]: image * scale against the float64 field at FIELD_ATOL x its rms
    (field key "image": against another z image / vol, given in place of the component).
    -> (largest integer distance, {name: max error / rms})."""
    volf = float(np.float32((L / N) ** 3))                     # the kernel's float32 cell volume
    if nx < N:
        sel = torch.nonzero((cells[:, 0] >= x0) & (cells[:, 0] < x0 + nx)).squeeze(1)
        cells, rho, vel = cells[sel], rho[sel], vel[sel]
    rows = _rows(N, nx, 1 << 26)
    dist = 0.0
    err, sq = {}, {}
    for i in range(0, nx, rows):
        j = min(nx, i + rows)
        s = chk.exact_slab_reference(cells, rho, vel, N, x0 + i, j - i)
        for img, c in integer:
            a = _invert_rows(img, N, nx, i, j).reshape(-1) / volf
            r = torch.round(a)
            _assert_equal_cells(r.to(torch.int64), s[1 + c], N, x0 + i, plan, "%s: sum rho v_%d" % (what, c))
            dist = max(dist, float((a - r).abs().max()))
            del a, r
        if real:
            f = chk.ngp_fields_float64(s[0].double(), [a.double() for a in s[1:]], (L / N) ** 3, ("velocity", "energy"))
            f["rv"] = [a.double() for a in s[1:]]
            for img, name, key, c, scale in real:
                ref = _invert_rows(c, N, nx, i, j).reshape(-1) / volf if key == "image" else f[key][c]
                got = _invert_rows(img, N, nx, i, j).reshape(-1) * scale
                err[name] = max(err.get(name, 0.0), float((got - ref).abs().max()))
                sq[name] = sq.get(name, 0.0) + float((ref * ref).sum())
                del got
            del f
        del s
    rel = {k: err[k] / np.sqrt(sq[k] / (nx * N * N)) for k in err}
    print("%s: largest distance from an integer %.3g; max error / rms %s" % (what, dist, {k: "%.3g" % v for k, v in rel.items()}))
    assert dist < INT_DIST, (what, dist)
    assert all(v < FIELD_ATOL for v in rel.values()), (what, rel)
    return dist, rel


def _check_momentum_images(K, N, n, dist, seed, x0=0, nx=None, **expect):
    from vpower import device
    nx = N if nx is None else nx
    if N in (250, 500) and not K.fused_supported(N, device.MOMENTUM):
        pytest.skip("the fused route does not take N = %d on this device (fused_supported)" % N)
    assert K.fused_supported(N, device.MOMENTUM), N
    L, cells, pos, rho, vel = _particles(K, n, N, dist, seed)
    plan = K.deposit_plan(pos.shape[0], 4, N, x0, nx, pencil=True)
    plan["x0"] = x0
    _expect(plan, bx=1, bz=N, **expect)
    _ran(plan, "pencil %d" % N, 4, pos)
    zimg = K.deposit_fft_z(pos, vel, rho, N, L, x0, nx, device.MOMENTUM)
    _check_images(K, N, L, x0, nx, cells, rho, vel, plan, "deposit_fft_z %d rows [%d, %d) %s" % (N, x0, x0 + nx, dist),
                  integer=[(zimg[c], c) for c in range(3)])
    del zimg
    _free(K)


@pytest.mark.parametrize("N,n", PENCILS)
def test_d_momentum_images_whole_grid(K, N, n):
    """Whole grids, uniform particles.  2048 (64-bit keys): 103 GB of z images + 4 GB of particles and cells + 6 GB of workspace
    + 4 GB of complex128 blocks and reference."""
    expect = {512: dict(wide_keys=0, cells_pow2=1), 2048: dict(wide_keys=1, two_level=1, staged=1), 384: dict(cells_pow2=0),
              768: dict(cells_pow2=0)}.get(N, {})
    _check_momentum_images(K, N, n, "uniform", 31, **expect)


@pytest.mark.parametrize("N,n", [(512, 10_000_000), (2048, 100_000_000)])
@pytest.mark.parametrize("dist", ["clump", "half_empty", "ends"])
def test_d_momentum_images_other_distributions(K, N, n, dist):
    _check_momentum_images(K, N, n, dist, 32, wide_keys=int(N == 2048))


def test_d_momentum_images_c5_share(K):
    """Rows 1536..2047 of 4096 from 1e9 replicated particles, twice.  First through the slab-sized workspace
    (vps_deposit_fft_z_slab: the compaction, 64-bit keys; its record arrays hold 1.3e8 entries, so only the INPUT arrays are
    indexed past 2^32 there).  Then through the plain workspace of vps_deposit_fft_z, whose key, rank and record arrays have
    one entry per particle: record word offsets cap_in * (C + 1) = 5e9 pass 2^32.
    40 GB of particles and cells + 103 GB of z images + 9 GB (then 54 GB) of workspace + 6 GB of blocks."""
    from vpower import device
    N, x0, nx, n = C5_SHARE
    L, cells, pos, rho, vel = _particles(K, n, N, "uniform", 33)
    inside = K.count_in_slab(pos, N, L, x0, nx)
    assert inside == int(((cells[:, 0] >= x0) & (cells[:, 0] < x0 + nx)).sum())
    plan = K.deposit_plan(n, 4, N, x0, nx, pencil=True, slab_particles=inside)
    plan["x0"] = x0
    _expect(plan, recompute=1, wide_keys=1, two_level=1, staged=1, bz=N)
    _ran(plan, "pencil 4096 slab", 4, pos)
    zimg = K.deposit_fft_z(pos, vel, rho, N, L, x0, nx, device.MOMENTUM, slab_particles=inside)
    _check_images(K, N, L, x0, nx, cells, rho, vel, plan, "deposit_fft_z_slab 4096 rows [1536, 2048)",
                  integer=[(zimg[c], c) for c in range(3)])
    _free(K)
    plan = K.deposit_plan(n, 4, N, x0, nx, pencil=True)
    plan["x0"] = x0
    _expect(plan, recompute=0, wide_keys=1, two_level=1, staged=1, cap_in=n)
    assert plan["cap_in"] * 5 >= 1 << 32                       # record word offsets beyond 32 bits
    _ran(plan, "pencil 4096 plain", 4, pos)
    zimg.zero_()
    K.deposit_fft_z(pos, vel, rho, N, L, x0, nx, device.MOMENTUM, zimg=zimg)
    del pos
    _check_images(K, N, L, x0, nx, cells, rho, vel, plan, "deposit_fft_z 4096 rows [1536, 2048), plain workspace",
                  integer=[(zimg[c], c) for c in range(3)])
    del zimg
    _free(K)


@pytest.mark.parametrize("N,n,x0,nx", [(512, 10_000_000, 0, 512), (2048, 100_000_000, 512, 1024)])
def test_d_velocity_energy_and_weighted_images(K, N, n, x0, nx):
    """The other launches of the pencil kernel on the same sort: the momentum launch that leaves the energy image behind
    (VPS_FLAG_SHARE_ENERGY), weighted_velocity with alpha = 1 against that momentum result / vol (both images inverted; the
    clump's cells are a thousand times the field's rms, so against the EXACT sums float32 rounding alone is 3600 x 2^-24 = 2e-4
    there: the two launches are compared with each other, as their contract says), then the energy launch and a velocity launch
    with VPS_FLAG_REUSE_SORT.  At 2048 on the rows 512..1535 (still 2^32 keys): the four momentum + energy images and the three
    weighted ones are 120 GB there, + 4 GB of particles and cells + 6 GB of workspace + 3 GB of blocks."""
    from vpower import device
    L, cells, pos, rho, vel = _particles(K, n, N, "clump", 34)
    plan = K.deposit_plan(n, 4, N, x0, nx, pencil=True)
    plan["x0"] = x0
    _expect(plan, wide_keys=int(N == 2048), two_level=1)
    _ran(plan, "pencil %d rows %d..%d" % (N, x0, x0 + nx - 1), 4, pos)
    what = "deposit_fft_z %d rows [%d, %d)" % (N, x0, x0 + nx)
    z4 = K.empty((4, K.zimage_elems(N, nx)), torch.complex64)
    K.deposit_fft_z(pos, vel, rho, N, L, x0, nx, device.MOMENTUM, flags=device.FLAG_SHARE_ENERGY, zimg=z4)
    _check_images(K, N, L, x0, nx, cells, rho, vel, plan, what + " momentum + shared energy",
                  integer=[(z4[c], c) for c in range(3)], real=[(z4[3], "E shared", "energy", 0, 1.0)])
    zw = K.deposit_fft_z(pos, vel, rho, N, L, x0, nx, device.WeightedVelocity(1.0))
    tok = K.fused_token()
    _check_images(K, N, L, x0, nx, cells, rho, vel, plan, what + " weighted velocity, alpha = 1, against momentum / vol",
                  real=[(zw[c], "w%d" % c, "image", z4[c], 1.0) for c in range(3)])
    del zw, z4
    torch.cuda.empty_cache()
    ze = K.deposit_fft_z(pos, vel, rho, N, L, x0, nx, device.ENERGY, reuse_sort=tok)
    tok = K.fused_token()
    _check_images(K, N, L, x0, nx, cells, rho, vel, plan, what + " energy (reused sort)", real=[(ze[0], "E", "energy", 0, 1.0)])
    del ze
    torch.cuda.empty_cache()
    zv = K.deposit_fft_z(pos, vel, rho, N, L, x0, nx, device.VELOCITY, reuse_sort=tok)
    _check_images(K, N, L, x0, nx, cells, rho, vel, plan, what + " velocity (reused sort)",
                  real=[(zv[c], "v%d" % c, "velocity", c, 1.0) for c in range(3)])
    del zv
    _free(K)


# ------------------------------------------------------------------------------------------- e ----
@pytest.mark.parametrize("opts", FLAVOURS, ids=lambda o: "%s=%d" % next(iter(o.items())))
def test_e_sort_flavours_at_2048(K, opts):
    """The 2048^3 one-channel deposit of b and the 2048 momentum images of d under each sort flavour; memory as there."""
    want = {"sort_atomic": dict(two_level=0), "sort_staged": dict(two_level=1, staged=0),
            "sort_groups": dict(two_level=1, staged=1, ngroups=4096)}[next(iter(opts))]
    with _options(opts):
        _check_raw_deposit(K, 2048, 1, 100_000_000, "uniform", 41, wide_keys=1, **want)
        if "sort_groups" in opts:
            assert K.deposit_plan(100_000_000, 4, 2048, 0, 2048, pencil=True)["staged_lds"] > 64 * 1024
        _check_momentum_images(K, 2048, 100_000_000, "clump", 42, wide_keys=1, **want)


# ------------------------------------------------------------------------------------------- f ----
def test_f_legs_ran_what_the_guard_counts(K):
    """Runs last, after the WHOLE file: the plans the legs actually ran (RAN) cover every plan leg a counted from the tables
    above, and the channel counts and position types the list asks for.  A partial run (-k, --lf, one leg alone) has not
    recorded every leg and fails here by design; the message says so."""
    from vpower import device
    whole = "(this check needs every leg of the file to have run in the same session: %d legs recorded)" % len(RAN)
    ran = {_flags(p) for p in RAN}
    for name, p in _matrix_plans(K).items():            # (_matrix_plans lists 250 / 500 only where the fused route takes them)
        assert _flags(p) in ran, ("no leg ran the plan of", name, p, whole)
    assert {p["C"] for p in RAN} == {1, 3, 4}, whole
    assert {p["dtype"] for p in RAN} == {"float32", "float64"}, whole
    assert any(p["cap_in"] * (p["C"] + 1) >= 1 << 32 for p in RAN), whole
    assert all(K.fused_supported(N, device.MOMENTUM) for N in (512, 1024, 2048, 384, 768))
