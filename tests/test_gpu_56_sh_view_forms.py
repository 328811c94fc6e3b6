"""-m gpu: the SH colour kernels at every coefficient count, degree and storage form, against the float64 restatement
(tests/sh_view_ref64.py; the dense pair against oracle.gs_oracle with float64 autograd).

Five one-view entries -- ``bds_sh_view_fwd``, ``bds_sh_view_bwd_list``, ``bds_view_grads_clear_list``, ``bds_view_grads_add_list``
(csrc/sh.hip) and ``bds_splat_pack_sh`` (csrc/rasterize.hip) -- and the dense pair ``bds_sh_fwd`` / ``bds_sh_bwd``, over
K in {1, 4, 5, 8, 9, 12, 16} x every degree with (deg+1)^2 <= K (17 pairs), the 16-byte vector and the scalar memory paths (K*3 % 4 and
a base pointer 4 bytes past a 16-byte boundary), the split storage of the reference's two parameters (``_features_dc`` [N,3] /
``_features_rest`` [N,K-1,3]: 16-byte accesses at 4-byte alignment for K*3 % 4 == 0, float by float otherwise), store and accumulate,
``row_map``, ``sh_rgb`` by Gaussian and by rank, a device-side list length, the 64-byte row form of the parameter gradients and
negative padding ids.

Shapes: N = 700 Gaussians (three 256-thread workgroups, the last one partial) and lists of 1 .. 513 entries on both sides of the
pack's 128-row and the other kernels' 256-row workgroups.  Every buffer a kernel sees is an exact-size body of
``tests.poison.poisoned_allocations``: a read past a row's end brings the guard's NaN into a result, a store past the end trips the
guard check, and every row a kernel must not touch is compared bit for bit with what was there before (the poison pattern for the
store forms, a fixed prior for the accumulate forms).

Tolerances are the project's for these operations (tests/test_gpu_01_gs_parity.py::test_sh_fwd_bwd): colours and coefficient-gradient
rows ``rel_err < 1e-5`` against float64, ``v_dirs < 1e-4`` for deg > 0; an accumulate onto a prior p is allowed one more float32
rounding of the sum, 2^-23 |p + ref|.

Two remarks on "bit for bit":
* accumulate-onto-zeros == store is asserted for a prior of NEGATIVE zeros, the additive identity of IEEE arithmetic (-0 + x has the
  bits of x for every x, -0 and +0 included).  The stored rows hold signed zeros (0 x a negative gradient in the unused bands and
  behind the clamp), and +0 + -0 = +0: onto positive zeros the two forms are equal as VALUES, which is asserted too.
* the clamp's outside neighbour at the upper end is sh_rgb = 0.5 + 2^-23 (sh_rgb + 0.5 = 1 + 2^-23 in float32).  nextafter(0.5)
  itself, 0.5 + 2^-24, sums to a tie that float32 rounds to exactly 1: it passes, as ``torch.clamp`` on the reference's float32
  colours passes it, and that is pinned as well."""
import pytest
import torch

from oracle import gs_oracle as G
from tests import sh_view_ref64 as R
from tests.poison import holds_poison, poisoned_allocations
from tests.util import rel_err

pytestmark = pytest.mark.gpu

N = 700
SENTINEL = 350                        # a Gaussian that is in no list: the padding id of the device-count forms
LIST_NS = (1, 127, 128, 129, 255, 256, 257, 513)
TOL, TOL_DIRS, EPS32 = 1e-5, 1e-4, 2.0 ** -23
SCHED_HEADER = 1 + 8 * 32             # csrc/rasterize.hip kSchedHeader: the words the record pack clears


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib as L
    L.lib()
    return L


@pytest.fixture(scope="module")
def data(env):
    """The inputs every case draws from (float32 on the device, never written)."""
    g = torch.Generator().manual_seed(56)
    d = dict(
        means=torch.randn(N, 3, generator=g) * 3,
        cam_pos=torch.randn(3, generator=g),
        dirs=torch.randn(N, 3, generator=g) * 2,
        sh=torch.randn(N, 16, 3, generator=g) * 1.2,            # (colours well beyond both ends of the clamp at every degree)
        v_out=torch.randn(N, 3, generator=g),
        masks=torch.rand(N, generator=g) > 0.2,
        radii=torch.randint(-3, 40, (N,), generator=g, dtype=torch.int32),
        depths=torch.rand(N, generator=g) * 10 + 0.1,
        m2=torch.rand(N, 2, generator=g) * 100,
        con=torch.rand(N, 3, generator=g) + 0.1,
        opac=torch.rand(N, generator=g),
        colors4=torch.rand(N, 4, generator=g),
        v_rec=torch.randn(max(LIST_NS), R.GRAD_RECORD_FLOATS, generator=g),
        perm=torch.randperm(N, generator=g).to(torch.int32),
        slots=torch.randperm(max(LIST_NS) + 5, generator=g).to(torch.int32),
    )
    d["masks"][0] = True
    # list order: random, the sentinel left out, and the array's last and first row in front -- every list holds the last row, whose
    # pieces end where the guard begins
    p = d["perm"]
    d["perm"] = torch.cat([torch.tensor([N - 1, 0], dtype=torch.int32), p[(p != SENTINEL) & (p != N - 1) & (p != 0)]])
    assert d["perm"].numel() == N - 1 and d["perm"].unique().numel() == N - 1
    d = {k: v.cuda() for k, v in d.items()}
    assert int((d["radii"] <= 0).sum()) > 20
    return d


# ---- exact-size poisoned buffers ---------------------------------------------------------------------------------------------------
def fresh(shape, off=0, dtype=torch.float32):
    """A poisoned body of exactly ``shape``; off = 1: it starts 4 bytes past a 16-byte boundary (a contiguous slice of a larger buffer)."""
    shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(n + off, dtype=dtype, device="cuda")
    body = buf[off:].view(shape)
    assert body.is_contiguous() and body.data_ptr() % 16 == 4 * off
    return body


def exact(t, off=0):
    """``t`` copied into an exact-size poisoned body."""
    body = fresh(tuple(t.shape), off, t.dtype)
    body.copy_(t)
    return body


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def rows_kept(out, prior, touched):
    """Rows of ``out`` outside ``touched`` (bool [rows]) hold the bits of ``prior`` (None: the poison pattern)."""
    rest = ~touched
    if prior is None:
        return bool(holds_poison(out[rest]).all())
    return torch.equal(bits(out[rest]), bits(prior[rest]))


def touched_mask(rows, dst):
    m = torch.zeros(rows, dtype=torch.bool, device="cuda")
    m[dst] = True
    return m


def list_ids(data, n):
    return data["perm"][:n].contiguous()


# ---- the dense pair ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,deg", R.K_DEG)
def test_dense_pair_aligned_and_offset(env, data, K, deg):
    """bds_sh_fwd / bds_sh_bwd against float64 autograd through the oracle, with and without masks, with and without v_dirs, on
    16-byte aligned bases and on bases 4 bytes past one (the scalar kernels at K in {4, 8, 12, 16}); both memory paths bit-equal."""
    L = env
    lib, st = L.lib(), L.stream()
    coeffs = data["sh"][:, :K].contiguous()
    for masked in (False, True):
        m = data["masks"] if masked else None
        d_ref = data["dirs"].double().requires_grad_(True)
        c_ref = coeffs.double().requires_grad_(True)
        ref = G.spherical_harmonics(deg, d_ref, c_ref, None if m is None else m.double())
        (ref * data["v_out"].double()).sum().backward()            # (rows are independent: the first n rows are the case of size n)
        for n in (1, 256, 257, 700):
            with poisoned_allocations(True, name=f"dense K={K} deg={deg} n={n} masked={masked}"):
                got = {}
                for off in (0, 1):
                    dirs, v_out = exact(data["dirs"][:n]), exact(data["v_out"][:n])
                    c_in = exact(coeffs[:n], off)
                    m_in = exact(m[:n].to(torch.uint8)) if masked else None
                    out = fresh((n, 3))
                    L.check(lib.bds_sh_fwd(n, K, deg, L.ptr(dirs), L.ptr(c_in), L.ptr(m_in), L.ptr(out), st), "sh fwd")
                    assert rel_err(out, ref[:n]) < TOL, (n, off, rel_err(out, ref[:n]))
                    res = [out]
                    for want_dirs in (False, True):
                        v_c = fresh((n, K, 3), off)
                        v_d = fresh((n, 3)) if want_dirs else None
                        L.check(lib.bds_sh_bwd(n, K, deg, L.ptr(dirs), L.ptr(c_in), L.ptr(m_in), L.ptr(v_out), L.ptr(v_c), L.ptr(v_d), st), "sh bwd")
                        assert rel_err(v_c, c_ref.grad[:n]) < TOL, (n, off, want_dirs, rel_err(v_c, c_ref.grad[:n]))
                        assert bool((v_c[:, R.num_bases(deg):] == 0).all())
                        if masked:
                            assert bool((v_c[~m[:n]] == 0).all()) and bool((out[~m[:n]] == 0).all())
                        res.append(v_c)
                        if want_dirs:
                            if deg > 0:
                                assert rel_err(v_d, d_ref.grad[:n]) < TOL_DIRS, (n, off, rel_err(v_d, d_ref.grad[:n]))
                            else:
                                assert bool((v_d == 0).all())           # a constant band has no direction gradient
                            res.append(v_d)
                    assert same_bits(res[1], res[2])                    # v_coeffs does not depend on whether v_dirs is asked for
                    got[off] = res
                for a, b in zip(got[0], got[1]):                        # same arithmetic, another memory path
                    assert same_bits(a, b), (n, masked)


# ---- bds_sh_view_fwd ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,deg", R.K_DEG)
def test_sh_view_fwd(env, data, K, deg):
    L = env
    lib, st = L.lib(), L.stream()
    coeffs = data["sh"][:, :K].contiguous()
    sh64 = R.colour64(deg, data["means"], data["cam_pos"], coeffs)
    for n in (1, 257, 700):
        vis = data["radii"][:n] > 0
        ref = sh64[:n] * vis[:, None]
        with poisoned_allocations(True, name=f"view fwd K={K} deg={deg} n={n}"):
            got = {}
            for off in (0, 1):
                means, cam, c_in = exact(data["means"][:n]), exact(data["cam_pos"]), exact(coeffs[:n], off)
                radii, dep = exact(data["radii"][:n]), exact(data["depths"][:n])
                sh_rgb, colors = fresh((n, 3)), fresh((n, 4))
                L.check(lib.bds_sh_view_fwd(n, K, deg, L.ptr(means), L.ptr(cam), L.ptr(c_in), L.ptr(radii), L.ptr(dep), L.ptr(sh_rgb),
                                            L.ptr(colors), st), "sh view fwd")
                assert rel_err(sh_rgb, ref) < TOL, (n, off, rel_err(sh_rgb, ref))
                assert same_bits(colors[:, :3], R.packed_colour(sh_rgb)) and same_bits(colors[:, 3], data["depths"][:n])
                assert bool((bits(sh_rgb[~vis]) == 0).all())                                        # culled: (0, 0, 0) ...
                assert bool((colors[~vis][:, :3] == 0.5).all())                                     # ... and (0.5, 0.5, 0.5, depth)
                got[off] = (sh_rgb, colors)
            assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])
    x = sh64[data["radii"] > 0] + 0.5
    assert bool((x < 0).any()) and bool((x > 1).any())                                              # the clamp is exercised at both ends


# ---- bds_splat_pack_sh -------------------------------------------------------------------------------------------------------------
def _pack_sh(L, n, n_dev, ids, K, deg, data, coeffs, rest, with_clears=True):
    """One run on fresh outputs; returns (code, records, sh_rgb_out, zero_records, zero_tail, schedule)."""
    lib, st = L.lib(), L.stream()
    inp = [exact(data[k]) for k in ("means", "cam_pos")]
    geo = [exact(data[k]) for k in ("m2", "con", "depths", "opac", "radii")]
    rec, sh_out = fresh((n, R.SPLAT_RECORD_FLOATS)), fresh((n, 3))
    zr, zt, sched = (fresh((n, R.GRAD_RECORD_FLOATS)), fresh(260), fresh(SCHED_HEADER + 43, dtype=torch.int32)) if with_clears else (None, None, None)
    code = lib.bds_splat_pack_sh(n, L.ptr(n_dev), L.ptr(ids), K, deg, L.ptr(inp[0]), L.ptr(inp[1]), L.ptr(coeffs), L.ptr(rest), L.ptr(geo[0]),
                                 L.ptr(geo[1]), L.ptr(geo[2]), L.ptr(geo[3]), L.ptr(geo[4]), L.ptr(rec), L.ptr(sh_out), L.ptr(zr), L.ptr(zt),
                                 260 if with_clears else 0, L.ptr(sched), st)
    return code, rec, sh_out, zr, zt, sched


def _pack_plain(L, n, n_dev, ids, data):
    """bds_splat_pack on the same geometry (any colours): the yardstick of the geometry slots and of what is cleared on the way."""
    lib, st = L.lib(), L.stream()
    geo = [exact(data[k]) for k in ("m2", "con", "colors4", "opac", "radii")]
    rec = fresh((n, R.SPLAT_RECORD_FLOATS))
    zr, zt, sched = fresh((n, R.GRAD_RECORD_FLOATS)), fresh(260), fresh(SCHED_HEADER + 43, dtype=torch.int32)
    L.check(lib.bds_splat_pack(n, L.ptr(n_dev), 4, L.ptr(ids), L.ptr(geo[0]), L.ptr(geo[1]), L.ptr(geo[2]), L.ptr(geo[3]), L.ptr(geo[4]), L.ptr(rec),
                               L.ptr(zr), L.ptr(zt), 260, L.ptr(sched), st), "pack")
    return rec, zr, zt, sched


def _check_pack(run, plain, m, n, ids, ref_rec, ref_rad, sh64_list, data):
    """Rows [0, m) against the restatement; rows [m, n) still poison; the clears as bds_splat_pack's."""
    code, rec, sh_out, zr, zt, sched = run
    p_rec, p_zr, p_zt, p_sched = plain
    assert code == 0
    if m:
        assert rel_err(sh_out[:m], sh64_list[:m]) < TOL, rel_err(sh_out[:m], sh64_list[:m])       # list order
        assert rel_err(rec[:m, 6:9], ref_rec[:m, 6:9]) < TOL
        assert same_bits(rec[:m, 6:9], R.packed_colour(sh_out[:m]))
        assert torch.equal(rec[:m, 9].double(), ref_rec[:m, 9])                                     # depth: a copy
        assert torch.equal(bits(rec[:m, 11]), ref_rad[:m])                                          # radius bits
        assert same_bits(rec[:m, :6], p_rec[:m, :6]) and bool((bits(rec[:m, 10]) == 0).all())       # geometry / opacity as the plain pack's
        assert rel_err(rec[:m, :6], ref_rec[:m, :6]) < TOL
    assert bool(holds_poison(rec[m:]).all()) and bool(holds_poison(sh_out[m:]).all())
    assert same_bits(zr, p_zr) and same_bits(zt, p_zt) and torch.equal(sched, p_sched)
    assert bool((bits(zr[:m]) == 0).all()) and bool(holds_poison(zr[m:]).all()) and bool((bits(zt) == 0).all())
    assert bool((sched[:SCHED_HEADER] == 0).all()) and bool(holds_poison(sched[SCHED_HEADER:]).all())


@pytest.mark.parametrize("K,deg", [kd for kd in R.K_DEG if kd[0] >= 2])
def test_splat_pack_sh_one_array_and_split(env, data, K, deg):
    """One-array form at K in {4, 8, 12, 16}, split form at every K >= 2; the two bit-equal; a device count below the capacity leaves
    the rows past it alone.  Where K = (deg+1)^2 the last piece of a split row ends at the row's end: at (4,1) and (16,3) it is a whole
    16-byte load whose last float is the row's last (one float further lies the next row, or behind the last row the guard's NaN);
    the float-by-float tail piece runs at (9,2) only, the one count whose 27 floats are no multiple of 4."""
    L = env
    coeffs = data["sh"][:, :K].contiguous()
    dc_t, rest_t = R.split_rows(coeffs)
    for n in LIST_NS:
        for m in ((n,) if n not in (129, 513) else (n, 2 * n // 3)):
            ids_t = list_ids(data, n).clone()
            ids_t[m:] = SENTINEL
            il = ids_t.long()
            sh64_list = R.colour64(deg, data["means"][il], data["cam_pos"], coeffs[il])
            ref_rec, ref_rad = R.splat_records(ids_t, data["m2"], data["con"], data["opac"], data["depths"], data["radii"], sh64_list)
            with poisoned_allocations(True, name=f"pack sh K={K} deg={deg} n={n} m={m}"):
                ids = exact(ids_t)
                n_dev = exact(torch.tensor([m], dtype=torch.int64, device="cuda")) if m != n else None
                plain = _pack_plain(L, n, n_dev, ids, data)
                runs = {}
                if K % 4 == 0:
                    runs["one"] = _pack_sh(L, n, n_dev, ids, K, deg, data, exact(coeffs), None)
                runs["split"] = _pack_sh(L, n, n_dev, ids, K, deg, data, exact(dc_t), exact(rest_t))
                for run in runs.values():
                    _check_pack(run, plain, m, n, ids_t, ref_rec, ref_rad, sh64_list, data)
                if len(runs) == 2:
                    assert same_bits(runs["one"][1][:m], runs["split"][1][:m]) and same_bits(runs["one"][2][:m], runs["split"][2][:m])


def test_splat_pack_sh_contract(env, data):
    """What the entry refuses: the split storage at K = 1, and the one-array storage with K*3 no multiple of 4 or rows off 16 bytes."""
    L = env
    with poisoned_allocations(True, name="pack sh contract"):
        ids = exact(list_ids(data, 129))
        for K, deg, split, off in ((1, 0, True, 0), (1, 0, False, 0), (5, 1, False, 0), (9, 2, False, 0), (4, 1, False, 1)):
            coeffs = data["sh"][:, :K].contiguous()
            dc_t, rest_t = (R.split_rows(coeffs) if K > 1 else (coeffs[:, 0].contiguous(), data["sh"][:, 1:2].contiguous()))
            args = (exact(dc_t), exact(rest_t)) if split else (exact(coeffs, off), None)
            code, rec, sh_out, _, _, _ = _pack_sh(L, 129, None, ids, K, deg, data, args[0], args[1], with_clears=False)
            assert code == L.BDS_EINVAL, (K, deg, split, off, code)
            assert bool(holds_poison(rec).all()) and bool(holds_poison(sh_out).all())               # nothing was launched


# ---- bds_sh_view_bwd_list ----------------------------------------------------------------------------------------------------------
def _bwd_list(L, n, n_dev, ids, K, deg, means, cam, sh_rgb, by_rank, v_rec, v_coeffs, v_rest, row_map, acc):
    return L.lib().bds_sh_view_bwd_list(n, L.ptr(n_dev), L.ptr(ids), K, deg, L.ptr(means), L.ptr(cam), L.ptr(sh_rgb), int(by_rank), L.ptr(v_rec),
                                        L.ptr(v_coeffs), L.ptr(v_rest), L.ptr(row_map), int(acc), L.stream())


def _forms(K):
    """(name, storage, base offset): what the entry's dispatch can take for this K."""
    f = [("one-array", "one", 0), ("one-array, offset base", "one", 1)]
    if K >= 2:
        f.append(("split", "split", 0))
    return f


def _run_bwd_list(L, K, deg, storage, off, rows, prior, n, n_dev, ids, means, cam, sh_rgb, by_rank, v_rec, row_map, acc):
    """One call on buffers of ``rows`` rows holding ``prior`` [rows,K,3] (None: poison); returns the result joined to [rows,K,3]."""
    if storage == "one":
        v_c = fresh((rows, K, 3), off) if prior is None else exact(prior, off)
        L.check(_bwd_list(L, n, n_dev, ids, K, deg, means, cam, sh_rgb, by_rank, v_rec, v_c, None, row_map, acc), "bwd list")
        return v_c
    if prior is None:
        dc, rest = fresh((rows, 3)), fresh((rows, K - 1, 3))
    else:
        dc, rest = (exact(t) for t in R.split_rows(prior))
    L.check(_bwd_list(L, n, n_dev, ids, K, deg, means, cam, sh_rgb, by_rank, v_rec, dc, rest, None, acc), "bwd list, split")
    return R.join_rows(dc, rest)


def _check_rows(out, prior, dst, rows64, nb, acc):
    """The listed rows against the restatement, everything else bit for bit what it was."""
    got = out[dst]
    if acc:
        want = prior[dst].double() + rows64
        bound = TOL * float(rows64.abs().max()) + EPS32 * want.abs()
        assert bool(((got.double() - want).abs() <= bound).all()), float(((got.double() - want).abs() - bound).max())
        assert same_bits(got[:, nb:], prior[dst][:, nb:])                     # bands >= nb: p + 0
    else:
        assert rel_err(got, rows64) < TOL, rel_err(got, rows64)
        assert bool((got[:, nb:] == 0).all())                                 # bands >= nb: exact zeros
    assert rows_kept(out, prior, touched_mask(out.shape[0], dst))


@pytest.mark.parametrize("K,deg", R.K_DEG)
def test_sh_view_bwd_list_forms(env, data, K, deg):
    """Storage form x store / accumulate x sh_rgb by Gaussian / by rank x row_map, at every list length."""
    L = env
    nb = R.num_bases(deg)
    g = torch.Generator().manual_seed(K * 10 + deg)
    sh_full = (torch.randn(N, 3, generator=g) * 0.6).cuda()                   # the forward's un-clamped colours: any values decide the clamp
    for n in LIST_NS:
        ids_t = list_ids(data, n)
        il = ids_t.long()
        rows64 = R.coeff_grad_rows(K, deg, data["means"][il], data["cam_pos"], data["v_rec"][:n], sh_full[il])
        map_rows = n + 5
        row_map_t = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        row_map_t[il] = data["slots"][data["slots"] < map_rows][:n]           # distinct rows of a compact exchange buffer
        with poisoned_allocations(True, name=f"bwd list K={K} deg={deg} n={n}"):
            ids, means, cam, v_rec = exact(ids_t), exact(data["means"]), exact(data["cam_pos"]), exact(data["v_rec"][:n])
            sh_by = {False: exact(sh_full), True: exact(sh_full[il])}
            row_map = exact(row_map_t)
            for mapped in (False, True):
                rows = map_rows if mapped else N
                dst = R.destination_rows(ids_t, row_map_t if mapped else None)
                prior = (torch.randn(rows, K, 3, generator=g) * 0.5).cuda()
                neg0 = torch.full((rows, K, 3), -0.0, device="cuda")
                for by_rank in (False, True):
                    res = {}
                    for name, storage, off in _forms(K):
                        if mapped and storage == "split":
                            continue                                          # (row_map is one-array only: pinned below)
                        a = (L, K, deg, storage, off, rows)
                        b = (n, None, ids, means, cam, sh_by[by_rank], by_rank, v_rec, row_map if mapped else None)
                        store = _run_bwd_list(*a, None, *b, 0)
                        _check_rows(store, None, dst, rows64, nb, False)
                        accum = _run_bwd_list(*a, prior, *b, 1)
                        _check_rows(accum, prior, dst, rows64, nb, True)
                        on0 = _run_bwd_list(*a, neg0, *b, 1)
                        assert same_bits(on0[dst], store[dst]) and rows_kept(on0, neg0, touched_mask(rows, dst)), (name, n)
                        on_pos0 = _run_bwd_list(*a, torch.zeros_like(neg0), *b, 1)
                        assert torch.equal(on_pos0[dst], store[dst]), (name, n)
                        res[name] = (store[dst], accum)
                    first = res["one-array"]
                    for name, r in res.items():                               # vector / scalar / split: the same bits
                        assert same_bits(r[0], first[0]) and same_bits(r[1], first[1]), (name, n, mapped, by_rank)
            if K >= 2:                                                        # the split storage takes no row_map
                dc, rest = fresh((N, 3)), fresh((N, K - 1, 3))
                assert _bwd_list(L, n, None, ids, K, deg, means, cam, sh_by[False], 0, v_rec, dc, rest, row_map, 0) == L.BDS_EINVAL
                assert bool(holds_poison(dc).all()) and bool(holds_poison(rest).all())
            else:                                                             # K = 1: a rest pointer is ignored
                dc, rest = fresh((N, 1, 3)), fresh((4,))
                L.check(_bwd_list(L, n, None, ids, K, deg, means, cam, sh_by[False], 0, v_rec, dc, rest, None, 0), "K = 1 with a rest pointer")
                _check_rows(dc, None, il, rows64, nb, False)
                assert bool(holds_poison(rest).all())


@pytest.mark.parametrize("K,deg", R.K_DEG)
def test_sh_view_bwd_list_device_count(env, data, K, deg):
    """The list length read from device memory: entries past it (padded with the sentinel's id) write nothing, not even the
    sentinel's rows."""
    L = env
    nb = R.num_bases(deg)
    g = torch.Generator().manual_seed(K * 10 + deg + 500)
    sh_full = (torch.randn(N, 3, generator=g) * 0.6).cuda()
    prior = (torch.randn(N, K, 3, generator=g) * 0.5).cuda()
    for n in (1, 129, 257, 513):
        m = 2 * n // 3
        ids_t = list_ids(data, n).clone()
        ids_t[m:] = SENTINEL
        il = ids_t[:m].long()
        rows64 = R.coeff_grad_rows(K, deg, data["means"][il], data["cam_pos"], data["v_rec"][:m], sh_full[il])
        sh_rank_t = sh_full[ids_t.long()]
        with poisoned_allocations(True, name=f"bwd list, device count K={K} deg={deg} n={n}"):
            ids, means, cam, v_rec = exact(ids_t), exact(data["means"]), exact(data["cam_pos"]), exact(data["v_rec"][:n])
            n_dev = exact(torch.tensor([m], dtype=torch.int64, device="cuda"))
            for by_rank, sh_rgb in ((False, exact(sh_full)), (True, exact(sh_rank_t))):
                for name, storage, off in _forms(K):
                    for acc, pr in ((0, None), (1, prior)):
                        out = _run_bwd_list(L, K, deg, storage, off, N, pr, n, n_dev, ids, means, cam, sh_rgb, by_rank, v_rec, None, acc)
                        if m:
                            _check_rows(out, pr, il, rows64, nb, bool(acc))
                        else:
                            assert rows_kept(out, pr, torch.zeros(N, dtype=torch.bool, device="cuda"))
                        assert rows_kept(out, pr, ~(torch.arange(N, device="cuda") == SENTINEL))     # the sentinel's rows (dc and rest)


@pytest.mark.parametrize("K,deg", [(1, 0), (4, 1), (5, 1), (9, 2), (12, 2), (16, 3)])
def test_sh_view_bwd_list_clamp_boundaries(env, data, K, deg):
    """sh_rgb planted at the clamp's ends: exactly -0.5 and 0.5 pass the gradient, the float32 neighbours outside give exact zeros."""
    L = env
    nb = R.num_bases(deg)
    n = 129
    ids_t = list_ids(data, n)
    il = ids_t.long()
    f32 = dict(dtype=torch.float32, device="cuda")
    lo, hi = torch.tensor(-0.5, **f32), torch.tensor(0.5, **f32)
    below = torch.nextafter(lo, torch.tensor(-1.0, **f32))
    above = torch.nextafter(torch.tensor(1.0, **f32), torch.tensor(2.0, **f32)) - hi          # sh_rgb + 0.5 = 1 + 2^-23
    tie = torch.nextafter(hi, torch.tensor(1.0, **f32))                                       # sh_rgb + 0.5 rounds to exactly 1
    sh_rank_t = torch.zeros(n, 3, **f32)
    sh_rank_t[0] = torch.stack([lo, hi, lo])             # all three pass
    sh_rank_t[1] = torch.stack([below, above, below])    # an exact zero row
    sh_rank_t[2] = torch.stack([below, hi, above])       # per channel
    sh_rank_t[128] = torch.stack([tie, above, lo])       # (the second workgroup's only entry)
    want_pass = torch.ones(n, 3, dtype=torch.bool, device="cuda")
    want_pass[1] = False
    want_pass[2] = torch.tensor([False, True, False], device="cuda")
    want_pass[128] = torch.tensor([True, False, True], device="cuda")
    assert torch.equal(R.clamp_pass(sh_rank_t), want_pass)
    sh_full_t = torch.zeros(N, 3, **f32)
    sh_full_t[il] = sh_rank_t
    rows64 = R.coeff_grad_rows(K, deg, data["means"][il], data["cam_pos"], data["v_rec"][:n], sh_rank_t)
    with poisoned_allocations(True, name=f"bwd list, clamp K={K} deg={deg}"):
        ids, means, cam, v_rec = exact(ids_t), exact(data["means"]), exact(data["cam_pos"]), exact(data["v_rec"][:n])
        for by_rank, sh_rgb in ((False, exact(sh_full_t)), (True, exact(sh_rank_t))):
            for name, storage, off in _forms(K):
                out = _run_bwd_list(L, K, deg, storage, off, N, None, n, None, ids, means, cam, sh_rgb, by_rank, v_rec, None, 0)
                _check_rows(out, None, il, rows64, nb, False)
                got = out[il]
                assert bool((got[1] == 0).all()), name
                for r in (0, 2, 128):
                    for ch in range(3):
                        assert bool((got[r, :nb, ch] != 0).all()) == bool(want_pass[r, ch]), (name, r, ch)
                        assert bool((got[r, :, ch] == 0).all()) == (not bool(want_pass[r, ch])), (name, r, ch)


# ---- bds_view_grads_clear_list / bds_view_grads_add_list ----------------------------------------------------------------------------
SHAPES5 = ((3,), (4,), (3,), ())          # v_means, v_quats, v_log_scales, v_logits (v_sh: [K,3])


def _padded_ids(data, n):
    """The list with padding -1 entries interleaved (every third entry)."""
    ids_t = list_ids(data, n).clone()
    ids_t[2::3] = -1
    return ids_t


def _clear(L, n, n_dev, ids, K, p5, g2, a2):
    return L.lib().bds_view_grads_clear_list(n, L.ptr(n_dev), L.ptr(ids), K, *p5, L.ptr(g2), L.ptr(a2), L.stream())


@pytest.mark.parametrize("K", [1, 4, 9, 16])
def test_view_grads_clear_list(env, data, K):
    """buf[ids] = 0 for the five arrays (and the screen-space pair), for the [N,16] row form, for the screen-space-only call and
    with a device count: every other row keeps its bits."""
    L = env
    g = torch.Generator().manual_seed(K)
    prior5 = [torch.randn(N, *s, generator=g).cuda() for s in SHAPES5] + [torch.randn(N, K, 3, generator=g).cuda()]
    prior2 = [torch.randn(N, 2, generator=g).cuda() for _ in range(2)]
    block_t = torch.randn(N, 16, generator=g).cuda()

    def cleared(t, il):
        t = t.clone()
        t[il] = 0
        return t

    for n in LIST_NS:
        ids_t = _padded_ids(data, n)
        il = ids_t[ids_t >= 0].long()
        with poisoned_allocations(True, name=f"clear list K={K} n={n}"):
            ids = exact(ids_t)
            for off in (0, 1):
                # the five separate arrays + the screen-space pair
                bufs = [exact(t) for t in prior5[:4]] + [exact(prior5[4], off)]
                g2, a2 = exact(prior2[0]), exact(prior2[1])
                L.check(_clear(L, n, None, ids, K, [L.ptr(b) for b in bufs], g2, a2), "clear list")
                for b, p in zip(bufs + [g2, a2], prior5 + prior2):
                    assert same_bits(b, cleared(p, il)), (n, off, tuple(p.shape))
                # the row form: the whole 64-byte row
                block, v_sh = exact(block_t), exact(prior5[4], off)
                base = L.ptr(block)
                L.check(_clear(L, n, None, ids, K, [base, base + 16, base + 32, base + 12, L.ptr(v_sh)], None, None), "clear list, row form")
                assert same_bits(block, cleared(block_t, il)) and same_bits(v_sh, cleared(prior5[4], il)), (n, off)
            # the screen-space-only call
            for pair in ((True, True), (False, True), (True, False)):
                g2, a2 = (exact(prior2[0]) if pair[0] else None), (exact(prior2[1]) if pair[1] else None)
                L.check(_clear(L, n, None, ids, K, [None] * 5, g2, a2), "clear list, screen space only")
                for b, p in ((g2, prior2[0]), (a2, prior2[1])):
                    assert b is None or same_bits(b, cleared(p, il)), (n, pair)
            # a device count: the entries past it are padded with the sentinel's id
            m = 2 * n // 3
            pad_t = ids_t.clone()
            pad_t[m:] = SENTINEL
            il_m = pad_t[:m][pad_t[:m] >= 0].long()
            ids_m, n_dev = exact(pad_t), exact(torch.tensor([m], dtype=torch.int64, device="cuda"))
            for off in (0, 1):
                bufs = [exact(t) for t in prior5[:4]] + [exact(prior5[4], off)]
                g2 = exact(prior2[0])
                L.check(_clear(L, n, n_dev, ids_m, K, [L.ptr(b) for b in bufs], g2, None), "clear list, device count")
                for b, p in zip(bufs + [g2], prior5 + prior2[:1]):
                    assert same_bits(b, cleared(p, il_m)), (n, off, tuple(p.shape))


@pytest.mark.parametrize("K", [1, 4, 9, 16])
def test_view_grads_add_list(env, data, K):
    """dst[ids] += src, one float32 add per element: exactly torch's indexed add; padding ids skipped, other rows untouched."""
    L = env
    lib, st = L.lib(), L.stream()
    g = torch.Generator().manual_seed(K + 100)
    shapes = list(SHAPES5) + [(K, 3)]
    prior = [torch.randn(N, *s, generator=g).cuda() for s in shapes]
    for n in LIST_NS:
        ids_t = _padded_ids(data, n)
        keep = ids_t >= 0
        il = ids_t[keep].long()
        src_t = [torch.randn(n, *s, generator=g).cuda() for s in shapes]
        want = []
        for p, s in zip(prior, src_t):
            w = p.clone()
            w[il] = w[il] + s[keep]
            want.append(w)
        with poisoned_allocations(True, name=f"add list K={K} n={n}"):
            ids = exact(ids_t)
            for off_dst, off_src in ((0, 0), (1, 0), (0, 1), (1, 1)):
                src = [exact(t) for t in src_t[:4]] + [exact(src_t[4], off_src)]
                dst = [exact(t) for t in prior[:4]] + [exact(prior[4], off_dst)]
                L.check(lib.bds_view_grads_add_list(n, L.ptr(ids), K, *[L.ptr(t) for t in src], *[L.ptr(t) for t in dst], st), "add list")
                for d, w in zip(dst, want):
                    assert same_bits(d, w), (n, off_dst, off_src, tuple(w.shape))
