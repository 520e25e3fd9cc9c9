"""-m gpu: the surface mesh derivative's kernels (csrc/msdiff.hpp, dsdf_msd_jacobian / dsdf_msd_jvp / dsdf_msd_vjp) on
their own, through ctypes on hand-filled DsdfMsdMesh / DsdfMsdBand: a seeded synthetic band with masked rows, rows outside the domain
and vertices without a valid endpoint, against the fp64 specification of tests/msdiff_numpy.py (surface_spec: the entry rule and
voldiff_numpy.tangent) at bounds counted from the kernels, entry by entry.  Every form of the dense kernel gives the same bits; the
adjoint with more than one part and more than one LDS tile at once; the part boundary; the tangent's bits shared with dsdf_vd_jvp;
entries out of range under red zones; the empty mesh.  tests/test_msdiff_cpu.py shows on the CPU that these inputs carry the edges
and that every wrong variant of msdiff_numpy.VARIANTS misses the specification by more than a thousand bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import msdiff_numpy as mn, ws_guard

pytestmark = pytest.mark.gpu

CASES = mn.CASES
SCALE = np.asarray(mn.SPACING, dtype=np.float32) / 2
# what the host's rule must select per case: (VEC, vertices per workgroup) of the compact and of the full form
FORMS = {"deg131_L2": ((1, 34), (1, 11)), "deg111_L4": ((4, 64), (4, 64)), "deg313_L27": ((1, 1), (1, 1)), "deg313_L128": ((4, 1), (4, 1))}
MISALIGNED_FORMS = {"deg111_L4": ((1, 64), (1, 21)), "deg313_L128": ((1, 1), (1, 1))}


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dense_form(ncp, L, full, aligned=True):
    """dsdf_msd_jacobian's rule, restated: float4 stores iff L % 4 == 0 and jac is 16-byte aligned; one vertex per workgroup when
    its stores reach MSD_DENSE_STORES, else as many as make that number, at most MSD_DENSE_VERTS."""
    K = ws_guard.constants()
    vec = 4 if L % 4 == 0 and aligned else 1
    stores = ncp * (L // vec) * (3 if full else 1)
    return vec, 1 if stores >= K["MSD_DENSE_STORES"] else min(K["MSD_DENSE_VERTS"], K["MSD_DENSE_STORES"] // stores)


class Surface:
    """A grid, an edge list and a band on the host (for the oracle) and on the device (for the kernels)."""

    def __init__(self, grid, case, edges=None, sb=None, first=None):
        self.grid, self.case = grid, case
        self.degrees, self.n_cp, self.L = CASES[case]
        self.ep, self.ea = mn.edges(grid) if edges is None else edges
        self.sb = mn.surface_band(grid.shape, self.ep, self.ea, self.degrees, self.n_cp, self.L) if sb is None else sb
        if first is not None:                                    # the first vertices of the list, the band of the whole list
            self.ep, self.ea = self.ep[:first], self.ea[:first]
        self.V, self.ncp = len(self.ep), int(np.prod(self.n_cp))
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        self.dev = dict(grid=cu(grid), ep=cu(self.ep.astype(np.int64)), ea=cu(self.ea.astype(np.int32)),
                        **{k: cu(self.sb[k]) for k in ("band_of", "G", "weights", "base", "mask")})

    def band_struct(self):
        from deepsdf_amd import _lib
        d, b = self.dev, _lib.DsdfMsdBand()
        b.G, b.weights, b.base, b.mask = (d[k].data_ptr() for k in ("G", "weights", "base", "mask"))
        b.n_band, b.ld_g, b.L = d["G"].shape[0], d["G"].stride(0), self.L
        for a in range(3):
            b.degree[a], b.n_cp[a] = self.degrees[a], self.n_cp[a]
        return b

    def structs(self, n_verts=None):
        from deepsdf_amd import _lib
        d, m = self.dev, _lib.DsdfMsdMesh()
        m.grid, m.edge_point, m.edge_axis, m.band_of = (d[k].data_ptr() for k in ("grid", "ep", "ea", "band_of"))
        m.n_verts, m.level = self.V if n_verts is None else n_verts, 0.0
        for a in range(3):
            m.dims[a], m.scale[a] = self.grid.shape[a], float(SCALE[a])
        return m, self.band_struct()

    def volume_structs(self):
        """The same vertices as a volume mesh: vert_point = edge_point, vert_class = 1 << edge_axis, every vertex listed, no clamp."""
        from deepsdf_amd import _lib
        d, m = self.dev, _lib.DsdfVdMesh()
        self._vol = (torch.bitwise_left_shift(torch.ones_like(d["ea"]), d["ea"]), torch.arange(self.V, dtype=torch.int32, device="cuda"))
        m.grid, m.vert_point, m.band_of = d["grid"].data_ptr(), d["ep"].data_ptr(), d["band_of"].data_ptr()
        m.vert_class, m.vert_index = self._vol[0].data_ptr(), self._vol[1].data_ptr()
        m.n_verts, m.n_moving, m.level, m.t_clamp = self.V, self.V, 0.0, 0.0
        for a in range(3):
            m.dims[a], m.scale[a] = self.grid.shape[a], float(SCALE[a])
        return m, self.band_struct()

    def parts(self):
        from deepsdf_amd import _lib
        nb, parts = C.c_size_t(), C.c_int32()
        _lib.check(_lib.lib().dsdf_msd_vjp_workspace_bytes(self.V, self.ncp, self.L, C.byref(nb), C.byref(parts)))
        return nb.value, parts.value

    def jacobian(self, full=0, jac=None, axis=None):
        from deepsdf_amd import _lib
        shape = (self.V, 3, self.ncp, self.L) if full else (self.V, self.ncp, self.L)
        jac = torch.full(shape, float("nan"), device="cuda") if jac is None else jac
        axis = torch.full((self.V,), -7, dtype=torch.int32, device="cuda") if axis is None else axis
        m, b = self.structs()
        _lib.check(_lib.lib().dsdf_msd_jacobian(C.byref(m), C.byref(b), full, ws_guard.ptr(jac), ws_guard.ptr(axis), ws_guard.stream()))
        return jac, axis

    def jvp(self, dcp, out=None):
        from deepsdf_amd import _lib
        out = torch.full((self.V, 3), float("nan"), device="cuda") if out is None else out
        m, b = self.structs()
        _lib.check(_lib.lib().dsdf_msd_jvp(C.byref(m), C.byref(b), ws_guard.ptr(dcp), ws_guard.ptr(out), ws_guard.stream()))
        return out

    def volume_jvp(self, dcp):
        from deepsdf_amd import _lib
        out = torch.full((self.V, 3), float("nan"), device="cuda")
        m, b = self.volume_structs()
        _lib.check(_lib.lib().dsdf_vd_jvp(C.byref(m), C.byref(b), ws_guard.ptr(dcp), ws_guard.ptr(out), ws_guard.stream()))
        return out

    def vjp(self, gv, out=None, ws=None):
        from deepsdf_amd import _lib
        out = torch.full((self.ncp, self.L), float("nan"), device="cuda") if out is None else out
        nbytes = self.parts()[0]
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda") if ws is None else ws
        m, b = self.structs()
        _lib.check(_lib.lib().dsdf_msd_vjp(C.byref(m), C.byref(b), ws_guard.ptr(gv), ws_guard.ptr(out), ws_guard.ptr(ws), nbytes, ws_guard.stream()))
        return out

    def spec(self):
        return mn.surface_spec(self.grid, self.ep, self.ea, self.sb, self.degrees, self.n_cp, SCALE)


_GRID = mn.seeded_grid()
_SPECS = {}


def small(case):
    """(Surface, its specification) on the 6 x 5 x 4 grid; the specification is computed once per case and left unchanged."""
    S = Surface(_GRID, case)
    if case not in _SPECS:
        _SPECS[case] = S.spec()
    return S, _SPECS[case]


def check_contractions(S, spec, tag, first=None):
    """dsdf_msd_jvp and dsdf_msd_vjp against the fp64 contractions at the counted bounds; exact zeros off the edge axis and where
    nothing contributes; two calls, identical bytes.  Returns (worst jvp error / bound, worst vjp error / bound, the adjoint)."""
    w, dcp = mn.contraction_inputs(len(spec["axis"]), S.ncp, S.L)
    w = w[:S.V]
    c = mn.contractions(spec, w, dcp, first)
    x, gv = torch.from_numpy(dcp).cuda(), torch.from_numpy(w).cuda()
    got = S.jvp(x)
    assert np.array_equal(bits(got), bits(S.jvp(x)))
    want, mag = c["jvp"]
    off = np.ones((S.V, 3), dtype=bool)
    off[np.arange(S.V), spec["axis"][:S.V]] = False
    assert not bits(got)[off].any() and not bits(got)[mag == 0].any()                              # exact +0
    rj = mn.ratio(got.cpu().numpy(), want, mn.jvp_bound(S.degrees, S.L, mag))
    adj = S.vjp(gv)
    assert np.array_equal(bits(adj), bits(S.vjp(gv)))
    parts = S.parts()[1]
    assert parts == -(-S.V // ws_guard.constants()["MSD_VJP_VERTS"])
    want, mag = c["vjp"]
    assert not bits(adj)[mag == 0].any()
    rv = mn.ratio(adj.cpu().numpy(), want, mn.vjp_bound(c["n_terms"], parts, mag))
    print(f"{tag}: {S.V} vertices, {parts} parts; jvp worst error / bound {rj:.3f}, vjp worst error / bound {rv:.3f}")
    assert rj <= 1 and rv <= 1, tag
    return rj, rv, adj


# ---- a. the dense Jacobian against fp64, entry by entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_dense_jacobian_entry_by_entry_against_fp64(case):
    S, spec = small(case)
    assert (dense_form(S.ncp, S.L, 0), dense_form(S.ncp, S.L, 1)) == FORMS[case]
    jac, axis = S.jacobian(0)
    assert np.array_equal(axis.cpu().numpy(), S.ea)
    bound = mn.dense_bound(spec["Jabs"])
    assert not bits(jac)[bound == 0].any()                                                         # exact +0 where no term is non-zero
    r = mn.ratio(jac.cpu().numpy(), spec["J"], bound)
    print(f"{case}: dense Jacobian, {int((bound > 0).sum())} non-zero entries of {bound.size}, worst error / bound {r:.3f}")
    assert r <= 1 and (bound > 0).sum() > 1000


# ---- b. every form of the dense kernel gives the same bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_every_dense_form_gives_the_same_bits(case):
    S, _ = small(case)
    V, per = S.V, S.ncp * S.L
    F = ws_guard.Fences()
    jac, axis = S.jacobian(0, F.new("jac", (V, S.ncp, S.L)), F.new("axis", (V,), torch.int32))
    full, axis_f = S.jacobian(1, F.new("full", (V, 3, S.ncp, S.L)), F.new("axis_full", (V,), torch.int32))
    F.check(f"{case}: compact and full")
    a = axis.long()
    assert torch.equal(axis, axis_f)
    ar = torch.arange(V, device="cuda")
    assert np.array_equal(bits(full[ar, a]), bits(jac))                                            # plane axis[v]: the compact block
    others = torch.ones(V, 3, dtype=torch.bool, device="cuda")
    others[ar, a] = False
    assert not bits(full[others]).any() and bits(jac).any()                                        # the other two planes: +0
    if case not in MISALIGNED_FORMS:
        return
    assert (dense_form(S.ncp, S.L, 0, False), dense_form(S.ncp, S.L, 1, False)) == MISALIGNED_FORMS[case]
    for f, ref in ((0, jac), (1, full)):
        n = V * per * (3 if f else 1)
        buf = F.new(f"misaligned {f}", (n + 4,))                                                   # jac one float into a larger buffer
        out = buf[1:n + 1].view(ref.shape)
        assert out.data_ptr() % 16 == 4
        S.jacobian(f, out)
        F.check(f"{case}: misaligned, full = {f}")
        assert np.array_equal(bits(out), bits(ref))
        assert (bits(buf[:1]) == 0xA5A5A5A5).all() and (bits(buf[n + 1:]) == 0xA5A5A5A5).all()     # the floats around it: untouched


# ---- c. jvp and vjp against fp64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_jvp_and_vjp_against_the_fp64_oracle(case):
    S, spec = small(case)
    check_contractions(S, spec, case)


@pytest.mark.parametrize("case", ["deg131_L2", "deg313_L128"])
def test_jvp_and_vjp_with_two_parts_of_the_adjoint(case):
    """966 vertices: two parts; deg313_L128: two parts times two LDS tiles, both terms of the partial's address non-zero."""
    S = Surface(mn.seeded_grid((9, 9, 9)), case)
    K = ws_guard.constants()
    assert S.V == 966 > K["MSD_VJP_VERTS"] and S.parts()[1] == 2
    assert (S.ncp * S.L > K["MSD_VJP_TILE"]) == (case == "deg313_L128")
    check_contractions(S, S.spec(), f"9 x 9 x 9, {case}")


# ---- d. the part boundary -------------------------------------------------------------------------------------------------------------------
def test_the_adjoint_at_a_part_boundary():
    """512 vertices are one part, 513 are two, the second with vertex 512 alone: the first parts are the same sums, so the two results
    differ by vertex 512's contribution (its own fmas and factors: the adjoint's bound with parts = 0) and the one addition that
    joins the parts (one U of the whole sum)."""
    grid, case = mn.seeded_grid((9, 9, 9)), "deg131_L2"
    whole = Surface(grid, case)
    spec = whole.spec()
    got = {}
    for n in (512, 513):
        S = Surface(grid, case, sb=whole.sb, first=n)
        assert S.V == n and S.parts()[1] == n - 511
        got[n] = check_contractions(S, spec, f"first {n} vertices", first=n)[2].cpu().numpy().astype(np.float64)
    w, dcp = mn.contraction_inputs(whole.V, whole.ncp, whole.L)
    v = 512
    g = float(w[v, spec["axis"][v]])
    want, mag = g * spec["J"][v], abs(g) * spec["Jabs"][v]
    assert spec["end"][v].any() and np.abs(want).max() > 0                                         # vertex 512 contributes
    n_v = sum((spec["end"][v, e] & spec["support"][spec["row"][v, e]]).astype(np.int64) for e in range(2))
    bound = mn.vjp_bound(n_v, 0, mag) + mn.U * mn.contractions(spec, w, dcp, 513)["vjp"][1]
    r = mn.ratio(got[513] - got[512], want, bound)
    print(f"part boundary: (513 vertices) - (512 vertices) against vertex 512's contribution, worst error / bound {r:.3f}")
    assert r <= 1


# ---- e. the tangent's bits are the volume kernel's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_jvp_has_the_bits_of_the_volume_kernel_on_axis_edges(case):
    S, spec = small(case)
    _, dcp = mn.contraction_inputs(S.V, S.ncp, S.L)
    x = torch.from_numpy(dcp).cuda()
    sj, vj = S.jvp(x), S.volume_jvp(x)
    assert np.array_equal(bits(sj), bits(vj)) and bits(sj).any()
    assert (bits(sj).any(1) == spec["end"].any(1)).all()                                           # zero rows: no valid endpoint


# ---- f. entries out of range ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_out_of_range_entries_contribute_nothing_under_red_zones(case):
    """Every index on this path is checked before it is used as an address -- msd_vertex: the axis, then 0 <= p < npts, then p's
    index along the axis (so p + stride[a] < npts) before grid[p], grid[q], band_of[p], band_of[q]; msd_ends: 0 <= row < nb before
    mask[row] and base[row], 0 <= base < ncp and first + deg < n_cp before any control point is named; msd_slot: the offsets within
    0 .. deg before a weight slot -- and a refused vertex reads grad_verts at axis 0 .. 2 of its own row."""
    from deepsdf_amd import _lib
    clean, _ = small(case)
    bp, ba, bsb, touched, zero = mn.invalid_entries(_GRID, clean.ep, clean.ea, clean.sb, clean.degrees, clean.n_cp)
    S = Surface(_GRID, case, edges=(bp, ba), sb=bsb)
    spec = S.spec()
    V = S.V
    w, dcp = mn.contraction_inputs(V, S.ncp, S.L)
    x, gv = torch.from_numpy(dcp).cuda(), torch.from_numpy(w).cuda()
    want_jac, _ = clean.jacobian(0)
    want_jvp = clean.jvp(x)
    keep, gone = torch.from_numpy(~touched).cuda(), torch.from_numpy(zero).cuda()
    results = []
    with ws_guard.redzone():
        for fill in (0x00, 0xFF):
            nbytes = S.parts()[0]
            ws = ws_guard.poisoned(nbytes, fill)
            F = ws_guard.Fences()
            jac, axis = S.jacobian(0, F.new("jac", (V, S.ncp, S.L)), F.new("axis", (V,), torch.int32))
            full, _ = S.jacobian(1, F.new("full", (V, 3, S.ncp, S.L)), F.new("axis_full", (V,), torch.int32))
            dv = S.jvp(x, F.new("d_verts", (V, 3)))
            gc = S.vjp(gv, F.new("grad_cp", (S.ncp, S.L)), ws)
            ws_guard.assert_clean(ws, fill, "msd_vjp")
            rows, _ = _lib.ws_regions()
            assert [r[0] for r in rows] == ["msd_vjp_part"]
            F.check("msd_jacobian / msd_jvp / msd_vjp")
            results.append((jac.clone(), full.clone(), axis.clone(), dv.clone(), gc.clone()))
    c = mn.contractions(spec, w, dcp)
    wrong = mn.surface_spec(_GRID, bp, ba, bsb, S.degrees, S.n_cp, SCALE, variant="wrapped_edge_counts")
    cw = mn.contractions(wrong, w, dcp)
    for jac, full, axis, dv, gc in results:
        assert np.array_equal(axis.cpu().numpy(), spec["axis"])
        assert not bits(jac[gone]).any() and not bits(full[gone]).any() and not bits(dv[gone]).any()                  # exact zeros
        assert np.array_equal(bits(jac[keep]), bits(want_jac[keep])) and np.array_equal(bits(dv[keep]), bits(want_jvp[keep]))
        assert np.array_equal(bits(full[torch.arange(V, device="cuda"), axis.long()]), bits(jac))
        bound_d = mn.dense_bound(spec["Jabs"])
        assert not bits(jac)[bound_d == 0].any()
        bound_j, bound_v = mn.jvp_bound(S.degrees, S.L, c["jvp"][1]), mn.vjp_bound(c["n_terms"], S.parts()[1], c["vjp"][1])
        assert not bits(dv)[bound_j == 0].any() and not bits(gc)[bound_v == 0].any()
        rd, rj = mn.ratio(jac.cpu().numpy(), spec["J"], bound_d), mn.ratio(dv.cpu().numpy(), c["jvp"][0], bound_j)
        rv = mn.ratio(gc.cpu().numpy(), c["vjp"][0], bound_v)
        # the rule the kernels had (an edge at the last index of axis 1 or 2 wraps into the next row and counts) misses by far
        miss = [float((np.abs(g.cpu().numpy() - a) > 1e3 * b).sum()) for g, a, b in
                ((jac, wrong["J"], bound_d), (dv, cw["jvp"][0], bound_j), (gc, cw["vjp"][0], bound_v))]
        print(f"{case}: entries out of range, worst error / bound dense {rd:.3f}, jvp {rj:.3f}, vjp {rv:.3f}; entries farther than 1e3 "
              f"bounds from 'wrapped_edge_counts': dense {miss[0]:.0f}, jvp {miss[1]:.0f}, vjp {miss[2]:.0f}")
        assert rd <= 1 and rj <= 1 and rv <= 1
        assert min(miss) >= 1
    assert np.array_equal(bits(results[0][4]), bits(results[1][4]))                                # the workspace's fill does not show


# ---- g. the empty mesh --------------------------------------------------------------------------------------------------------------------------
def test_empty_mesh():
    from deepsdf_amd import _lib
    S, _ = small("deg131_L2")
    lib = _lib.lib()
    F = ws_guard.Fences()
    gc = F.new("grad_cp", (S.ncp, S.L))
    gc.fill_(float("nan"))
    jac, axis, dv = F.new("jac", (S.ncp, S.L)), F.new("axis", (4,), torch.int32), F.new("d_verts", (4, 3))
    before = [t.clone() for t in (jac, axis, dv)]
    m, b = S.structs(n_verts=0)
    null = C.c_void_p(0)
    assert lib.dsdf_msd_vjp(C.byref(m), C.byref(b), null, ws_guard.ptr(gc), null, 0, ws_guard.stream()) == 0
    for full in (0, 1):
        assert lib.dsdf_msd_jacobian(C.byref(m), C.byref(b), full, ws_guard.ptr(jac), ws_guard.ptr(axis), ws_guard.stream()) == 0
    assert lib.dsdf_msd_jvp(C.byref(m), C.byref(b), ws_guard.ptr(gc), ws_guard.ptr(dv), ws_guard.stream()) == 0
    F.check("empty mesh")
    assert not bits(gc).any()                                                                      # exact +0 everywhere
    for t, was in zip((jac, axis, dv), before):
        assert torch.equal(t.view(torch.uint8), was.view(torch.uint8))                             # nothing written
    nb, parts = C.c_size_t(), C.c_int32()
    assert lib.dsdf_msd_vjp_workspace_bytes(0, S.ncp, S.L, C.byref(nb), C.byref(parts)) == 0 and parts.value == 0
