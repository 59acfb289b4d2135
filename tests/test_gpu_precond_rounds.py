"""The preconditioned proposal kernel (capi.hip precond_propose_kernel) where one workgroup walks SEVERAL tiles.  Needs an
MI355X: run with `-m gpu`.

The kernel is a persistent loop, `for (tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)`: from its second iteration on a
workgroup meets the barrier at the top of the loop against the previous tile's copy-out, reuses the z and x slabs, and takes
`first = 64 tile` with tile != blockIdx.x - the rows, chains and temperatures of the Philox path included.  None of that runs
while the launch has one workgroup per tile, and the launcher gives it one up to G = 8 workgroups per compute unit
(precond.h prec_grid, restated as precond_reference.grid; tests/test_precond_host.py holds the two together): every batch of
tests/test_gpu_precond.py but one is a single round.

How the batches here make several rounds CERTAIN:
  * G = grid(any number of tiles, CUs) is the most workgroups a launch ever has (CUs: torch's multi_processor_count);
  * a batch has n_tiles = k G + r tiles, 0 < r < G: its launch has G workgroups and ceil(n_tiles / G) = k + 1 rounds, so every
    tile with index >= G is at least the SECOND tile of its workgroup and every tile >= 2 G at least the THIRD (the slabs
    reused behind a reuse);
  * r is no multiple of 4, so the last round is uneven - most workgroups have left the loop while some walk one tile more;
  * the last tile holds 5 rows: a partial tile in the last round, behind full ones in the same slabs;
  * with T = 3 or 5 temperatures the number of chains is chosen so that n_chains x T is exactly that row count; tiles then
    straddle chains, and row -> (chain, temperature) is taken at every offset.
Each case asserts the three facts from precond_reference.grid and its own row count alone: arithmetic on the inputs.  On a
256-CU device G = 2 048; the largest case, dim 104 with 133 445 rows, is 53 MiB per array.

What is compared: on integers - where every order of the sums gives the same floats - every row of the batch against the
float64 product on the host, with sentinels around the caller-owned arrays; on generic floats five blocks of 128 rows at the
seams of the rounds against precond_reference's fmaf chain, bit for bit; the Philox path, every row, against the same kernel
fed the Normal kernel's own normals.
"""
import numpy as np
import pytest
import torch

import precond_reference as PR
import ptrwm_hip as E

pytestmark = pytest.mark.gpu

HUGE = 1 << 40  # more tiles than any launch has workgroups
# case -> (dim, k, T).  dim 16: the accept uniform's Philox block lies behind the slab's columns; 17 and 33 open a block of 16
# with one coordinate; 104: the raised-LDS shape, one workgroup per compute unit
CASES = {"d5-T1-k2": (5, 2, 1), "d5-T3-k2": (5, 2, 3), "d30-T1-k2": (30, 2, 1), "d30-T5-k2": (30, 2, 5), "d16-T3-k1": (16, 1, 3),
         "d17-T1-k1": (17, 1, 1), "d33-T5-k1": (33, 1, 5), "d104-T1-k1": (104, 1, 1), "d104-T3-k1": (104, 1, 3)}
DEVICE_STEP_CASE = "d30-T5-k2"  # the Philox test of this shape reads its step from a counter in device memory
SENTINEL, PAD = 12345.0, 8  # floats around every caller-owned array (PAD floats keep a 16-byte boundary)


def plan_rounds(k, T, cus):
    """(G, r, n_tiles, n_chains) of a batch of k G + r tiles whose last tile holds 5 rows: the largest r <= 38 that is no
    multiple of 4 and makes the row count a multiple of T (64 is prime to 3 and 5: one of any T consecutive r does)."""
    G = PR.grid(HUGE, cus)
    for r in range(min(38, G - 1), 0, -1):
        n_rows = PR.ROWS * (k * G + r - 1) + 5
        if r % 4 != 0 and n_rows % T == 0:
            return G, r, k * G + r, n_rows // T
    raise AssertionError(f"no r for k = {k}, T = {T}, G = {G}")


def device_cus(device):
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    assert cus >= 2
    return cus


def shape_of(device, case):
    """dim, k, T, G, n_chains, n_rows of a case, with the three facts asserted from PR.grid alone"""
    dim, k, T = CASES[case]
    cus = device_cus(device)
    G, r, n_tiles, Cn = plan_rounds(k, T, cus)
    n_rows = Cn * T
    assert PR.tiles(n_rows) == n_tiles and PR.grid(n_tiles, cus) == G == PR.grid(HUGE, cus)
    assert -(-n_tiles // PR.grid(n_tiles, cus)) == k + 1 >= 2  # rounds
    assert 0 < n_tiles % G < G and (n_tiles % G) % 4 != 0  # the last round is uneven
    assert n_rows - PR.ROWS * (n_tiles - 1) == 5  # the last tile is partial
    return dim, k, T, G, Cn, n_rows


def row_ranges(n_rows, G):
    """[0, 64 G), [64 G, 128 G), [128 G, n_rows): rows of the first, second, third-or-later tile of a workgroup"""
    edges = [0] + [e for e in (PR.ROWS * G, 2 * PR.ROWS * G) if e < n_rows] + [n_rows]
    return list(zip(edges[:-1], edges[1:]))


def seam_blocks(n_rows, G, k):
    """First rows of five blocks of 128 rows: the first, the one straddling 64 G, the one straddling 128 G (k = 1: a quarter into
    the last range), the middle of the last range, the very last - which includes the 5-row tile."""
    last0 = row_ranges(n_rows, G)[-1][0]
    third = 2 * PR.ROWS * G - 64 if k == 2 else last0 + (n_rows - last0) // 4 - 64
    starts = [0, PR.ROWS * G - 64, third, (last0 + n_rows) // 2 - 64, n_rows - 128]
    assert all(0 <= a and a + 128 <= b for a, b in zip(starts, starts[1:] + [n_rows + 128])), starts  # in range, disjoint, ascending
    return starts


def guarded(device, shape, shift=0, dtype=torch.float32):
    """A contiguous view of `shape`, `shift` floats off a 16-byte boundary, inside its own sentinel-filled allocation"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * PAD + 4,), SENTINEL, device=device, dtype=dtype)
    view = flat[PAD + shift:PAD + shift + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * shift
    return flat, view


def guards_intact(flat, view):
    lo = (view.data_ptr() - flat.data_ptr()) // 4
    return bool((flat[:lo] == SENTINEL).all()) and bool((flat[lo + view.numel():] == SENTINEL).all())


def nan_upper(L):
    return (np.tril(L) + np.triu(np.full(L.shape, np.nan), 1)).astype(np.float32)


def random_factor(rng, dim, cond=100.0):
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    cov = (q * np.exp(np.linspace(0.0, np.log(cond), dim))) @ q.T
    return np.linalg.cholesky((cov + cov.T) / 2)


def make_plan(device, st, scales, chol, scratch=None, *, seed=0, chain_offset=0, **kw):
    """A plan for split steps on state `st` [C, T, D]; `chol`: the factor tensor bound (None: the plain Normal proposal);
    `scratch`: the caller's (proposals, accept_u), put where RunPlan._split_buffers() would put the plan's own."""
    Cn, T, D = st.shape
    prop = E.Proposal(E.PROPOSAL_NORMAL, torch.tensor(np.asarray(scales, np.float32), device=device))
    kw.setdefault("logp", torch.zeros(Cn, T, device=device))
    kw.setdefault("beta", torch.ones(T, device=device))
    plan = E.RunPlan(None, prop, state=st, seed=seed, chain_offset=chain_offset, **kw)
    if chol is not None:
        plan.set_preconditioner(chol)
    if scratch is not None:
        plan._split = tuple(scratch)
    return plan


def integer_batch(rng, dim, Cn, T):
    """The data of test_exact_layout_on_integers: integer z in [-4, 4], an integer asymmetric lower-triangular L in [-3, 3] with
    NaN above its diagonal, integer x, scales that are powers of two and differ per temperature - every product and partial sum
    is exact in float32 whatever the order - and the float64 product."""
    L = rng.integers(-3, 4, (dim, dim)).astype(np.float64)
    L[np.arange(dim), np.arange(dim)] = rng.integers(1, 4, dim)
    z = rng.integers(-4, 5, (Cn, T, dim)).astype(np.float32)
    x = rng.integers(-50, 51, (Cn, T, dim)).astype(np.float32)
    u = rng.random((Cn, T)).astype(np.float32)
    scales = np.float32(2.0) ** -np.arange(1, T + 1, dtype=np.float32)
    want = (x.astype(np.float64) + scales[None, :, None].astype(np.float64) * (z.astype(np.float64) @ np.tril(L).T)).astype(np.float32)
    return nan_upper(L), z, x, u, scales, want


def integers_on_guarded_arrays(device, dim, Cn, T, seed, state_shift=0, props_shift=0):
    """One external-randoms proposal on integer data with the state, the proposals and accept_u each inside its own
    sentinel-filled allocation, `state_shift` / `props_shift` floats off a 16-byte boundary: every row equals the float64
    product; plane 0 of accept_u is ext_u and plane 1 is -1; state and factor keep their bits; every sentinel is intact.
    Returns (proposals, x) as [rows, dim] host arrays."""
    rng = np.random.default_rng(seed)
    chol_np, z, x, u, scales, want = integer_batch(rng, dim, Cn, T)
    chol = torch.tensor(chol_np, device=device)
    sflat, st = guarded(device, (Cn, T, dim), state_shift)
    pflat, props = guarded(device, (Cn, T, dim), props_shift)
    aflat, acc = guarded(device, (2, Cn, T))
    xd = torch.tensor(x, device=device)
    st.copy_(xd)
    plan = make_plan(device, st, scales, chol, (props, acc))
    out = plan.split_propose(0, ext_prop=torch.tensor(z, device=device), ext_u=torch.tensor(u, device=device))
    torch.cuda.synchronize()
    assert out.data_ptr() == props.data_ptr() and plan._split_buffers()[1].data_ptr() == acc.data_ptr()
    what = (dim, Cn, T, state_shift, props_shift)
    got = props.cpu().numpy()
    assert not np.isnan(got).any(), what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5])
    a = acc.cpu().numpy()
    assert np.array_equal(a[0], u) and np.all(a[1] == -1.0), what
    assert torch.equal(st, xd), what  # the state is only read
    assert np.array_equal(chol.cpu().numpy().view(np.uint32), chol_np.view(np.uint32)), what  # ... and so is the factor
    assert guards_intact(sflat, st) and guards_intact(pflat, props) and guards_intact(aflat, acc), what
    return got.reshape(-1, dim), x.reshape(-1, dim)


@pytest.mark.parametrize("case", list(CASES))
def test_every_row_of_several_rounds_on_integers(device, case):
    """k G + r tiles (module docstring), external randoms, integer data: the whole batch equals x + s_t (z @ tril(L).T) computed
    in float64 on the host, plane 0 of accept_u equals ext_u and plane 1 is -1 for every row, state and factor are unchanged,
    the sentinels in front of and behind proposals, accept_u and the state are intact, and the rows of the first, second and
    (k = 2) third-or-later tile of a workgroup each differ from their x - no range passes by being skipped."""
    dim, k, T, G, Cn, n_rows = shape_of(device, case)
    got, x = integers_on_guarded_arrays(device, dim, Cn, T, seed=5000 + dim + T)
    ranges = row_ranges(n_rows, G)
    assert len(ranges) == k + 1
    moved = (got != x).any(axis=1)
    for a, b in ranges:
        assert moved[a:b].mean() > 0.9, (case, a, b)
    print(f"{case}: {n_rows} rows, {PR.tiles(n_rows)} tiles on {G} workgroups, {k + 1} rounds, {n_rows * dim * 4 / 2**20:.1f} MiB per array")


@pytest.mark.parametrize("case", list(CASES))
def test_the_rule_bit_for_bit_at_the_seams_of_the_rounds(device, case):
    """Generic floats drawn on the device - Gaussian z, a factor of condition about 100 with NaN above its diagonal, x of scale
    10, scales that differ per temperature: five blocks of 128 rows - the first, those straddling the first and the second
    round's end (k = 1: a quarter into the last round), the middle of the last round, and the last, with the 5-row tile -
    equal precond_reference's fmaf chain as floats."""
    dim, k, T, G, Cn, n_rows = shape_of(device, case)
    rng = np.random.default_rng(6000 + dim + T)
    g = torch.Generator(device=device)
    g.manual_seed(6000 + dim + T)
    chol_np = nan_upper(random_factor(rng, dim))
    z = torch.randn(Cn, T, dim, generator=g, device=device)
    x = 10.0 * torch.randn(Cn, T, dim, generator=g, device=device)
    u = torch.rand(Cn, T, generator=g, device=device)
    scales = np.linspace(0.7, 1.9, T).astype(np.float32)
    x0 = x.clone()
    plan = make_plan(device, x, scales, torch.tensor(chol_np, device=device))
    got = plan.split_propose(0, ext_prop=z, ext_u=u).view(-1, dim)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and not bool(torch.isnan(got).any())
    for a in seam_blocks(n_rows, G, k):
        rows = slice(a, a + 128)
        want = PR.propose_rows(x.view(-1, dim)[rows].cpu().numpy(), chol_np, z.view(-1, dim)[rows].cpu().numpy(),
                               scales[np.arange(a, a + 128) % T])
        have = got[rows].cpu().numpy()
        assert np.array_equal(have, want), (case, a, np.argwhere(have != want)[:5])


@pytest.mark.parametrize("case", list(CASES))
def test_philox_path_of_every_row_of_several_rounds(device, case):
    """The method of test_philox_path_against_the_normal_kernels_own_normals: ptrwm_split_propose with NormalProposal, unit
    scales and a zero state yields z and the accept uniforms of the same seed, step, chain_offset (above 2^33) and T.  The
    preconditioned kernel in Philox mode then equals THE SAME KERNEL fed that z as external randoms, over the whole batch on the
    device - the external path takes row i's normals from ext_prop + i dim, so a tile that drew the words of another row,
    chain or temperature differs - its plane 0 equals the Normal kernel's uniforms for every row, and the five seam blocks
    equal precond_reference on that z.  One shape reads its step from a counter in device memory."""
    dim, k, T, G, Cn, n_rows = shape_of(device, case)
    device_step = case == DEVICE_STEP_CASE
    rng = np.random.default_rng(7000 + dim + T)
    seed, step, offset = 0x1234567890ABCDEF, 41, (1 << 33) + 5
    counter = torch.tensor([step - 2], dtype=torch.int64, device=device) if device_step else None
    arg = 2 if device_step else step  # (device-step mode: the counter plus this call's offset)
    ref_plan = make_plan(device, torch.zeros(Cn, T, dim, device=device), np.ones(T, np.float32), None, seed=seed, chain_offset=offset)
    ref_plan.set_device_step(counter)
    z = ref_plan.split_propose(arg)
    u = ref_plan._split_buffers()[1][0]
    assert bool(torch.isfinite(z).all()) and 0.99 < float(z.std()) < 1.01
    g = torch.Generator(device=device)
    g.manual_seed(7000 + dim + T)
    chol_np = nan_upper(random_factor(rng, dim))
    chol = torch.tensor(chol_np, device=device)
    x = 10.0 * torch.randn(Cn, T, dim, generator=g, device=device)
    scales = np.linspace(0.5, 2.9, T).astype(np.float32)
    plan = make_plan(device, x, scales, chol, seed=seed, chain_offset=offset)
    plan.set_device_step(counter)
    got = plan.split_propose(arg)
    acc = plan._split_buffers()[1]
    fed = make_plan(device, x, scales, chol, seed=seed + 1, chain_offset=0)  # (external randoms: neither is looked at)
    got_fed = fed.split_propose(0, ext_prop=z, ext_u=u)
    torch.cuda.synchronize()
    assert torch.equal(got, got_fed), (case, torch.nonzero(got != got_fed)[:5].tolist())
    assert torch.equal(acc[0], u) and bool((acc[1] == -1.0).all()), case
    for a, b in row_ranges(n_rows, G):
        assert bool((got.view(-1, dim)[a:b] != x.view(-1, dim)[a:b]).any(dim=1).all()), (case, a, b)
    for a in seam_blocks(n_rows, G, k):
        rows = slice(a, a + 128)
        want = PR.propose_rows(x.view(-1, dim)[rows].cpu().numpy(), chol_np, z.view(-1, dim)[rows].cpu().numpy(),
                               scales[np.arange(a, a + 128) % T])
        have = got.view(-1, dim)[rows].cpu().numpy()
        assert np.array_equal(have, want), (case, a, np.argwhere(have != want)[:5])
    if device_step:
        assert int(counter.item()) == step - 2  # the proposal does not advance the counter
