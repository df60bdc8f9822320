"""-m gpu: the device side of the multi-rank path on ONE GPU. All ranks of a k-way partition live in
this process; a loopback transport copies each send chunk into the peer's receive chunk (what RCCL
send/recv does across GPUs). Exercises the HIP pack/unpack kernels, the ghost mirror slots and the
interior / ghost-reading tile split of the fused kernels; the gathered result must equal the
single-rank run."""
import numpy as np
import pytest
import torch

from _gpu import perturbed_state, rel_err
from t8gpu_amd.halo import HaloExchange
from t8gpu_amd.solver import PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu


def loopback(halos):
    """Deliver every rank's send chunks (all packs enqueued before, all unpacks after, same stream)."""
    by_rank = {h.rank: h for h in halos}
    for h in halos:
        for j, p in enumerate(h.peers):
            peer = by_rank[p]
            jj = peer.peers.index(h.rank)
            w = 5 * h.cells
            src = h.sendbuf[w * h.send_off[j]:w * h.send_off[j + 1]]
            dst = peer.recvbuf[w * peer.recv_off[jj]:w * peer.recv_off[jj + 1]]
            assert src.numel() == dst.numel() > 0
            dst.copy_(src)


@pytest.mark.parametrize("world", [2, 4, 7])
@pytest.mark.parametrize("mode", ["fused", "compat"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_k_way_partition_on_one_gpu_equals_single_rank(world, mode, dtype):
    k_way_plain(SynthMesh(2, 4, 7, band=0.06), world, mode, dtype, small_tiles=True)


@pytest.mark.parametrize("mode", ["fused", "compat"])
def test_more_ranks_than_elements(mode):
    """4 elements on 6 ranks: two ranks own nothing (no elements, faces, ghosts or peers) and every launch on them
    is a no-op; the others own one element whose neighbours are all ghosts."""
    mesh = SynthMesh(2, 1, 1)
    assert sorted(mesh.partition(r, 6).N for r in range(6)) == [0, 0, 1, 1, 1, 1]
    k_way_plain(mesh, 6, mode, torch.float64, small_tiles=False)
    if mode == "fused":                                         # the C++ step driver on a rank that owns nothing
        empty = PlainSolver(mesh.partition(0, 6), torch.float64, mode="fused")
        empty.use_native_stepper()
        empty.iterate(0.05)
        empty.iterate_steps(3, 0.05)
        torch.cuda.synchronize()
        assert tuple(empty.state().shape) == (5, 0) and empty.compute_integral(0) == 0.0


def k_way_plain(mesh, world, mode, dtype, small_tiles):
    whole = mesh.partition()
    st = perturbed_state(whole, 77)
    ref = PlainSolver(whole, dtype, mode=mode, state=st)
    parts = [mesh.partition(r, world) for r in range(world)]
    solvers, halos = [], []
    for part in parts:
        gidx = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        local = st[:, gidx].copy()
        local[:, part.N:] = np.nan                              # ghost values must arrive through the exchange
        solvers.append(PlainSolver(part, dtype, mode=mode, state=local))
        halos.append(HaloExchange(part, dtype, dist=None, overlap=False))
    if mode == "fused" and small_tiles:
        from t8gpu_amd import fused
        for s, part in zip(solvers, parts):                     # small tiles: interior AND ghost-reading tiles on every rank
            s.plan = fused.PlainPlan(part, dtype, tmax=32, fcap=80)
        assert all(0 < s.plan.host.n_interior < s.plan.host.ntiles for s in solvers)
    dt = 0.1 * 2.0 ** -mesh.finest_level
    for _ in range(3):
        ref.iterate(dt)
        for s in solvers:
            s.begin_step()
        for k in range(3):
            for s, h in zip(solvers, halos):
                h._pack(s.step_planes(s.stage_steps(k)[0]))
            loopback(halos)
            for s, h in zip(solvers, halos):
                h._unpack(s.step_planes(s.stage_steps(k)[0]))
            for s in solvers:
                s.run_stage(k, dt, split=True)
    torch.cuda.synchronize()
    full = torch.cat([s.state() for s in solvers], dim=1).cpu().numpy()
    assert not np.isnan(full).any()
    tol = 1e-13 if dtype == torch.float64 else 2e-6
    assert rel_err(full, ref.state().cpu().numpy()) < tol
    if mode == "fused":
        # fused sums run in face order on every rank: the partitioned run is BITWISE the single-rank run
        assert np.array_equal(full, ref.state().cpu().numpy())


def send_map_of(send_idx, n_owned):
    """T8gpuPlainPlan.send_map / send_list (include/t8gpu_hip.h, "ghost window") from a rank's send list."""
    smap = np.full(max(1, n_owned), -1, np.int32)
    slots = {}
    for t, e in enumerate(send_idx.tolist()):
        slots.setdefault(e, []).append(t)
    lst = []
    for e, ts in slots.items():
        if len(ts) == 1:
            smap[e] = ts[0]
        else:
            smap[e] = -(2 + len(lst))
            lst += ts[:-1] + [ts[-1] - 2 ** 31]
    return smap, np.asarray(lst if lst else [0], np.int64).astype(np.int32)


@pytest.mark.parametrize("world", [2, 5, 7])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tiles", ["small", "patches", "generic"])
def test_ghost_window_k_way_partition_equals_single_rank(world, dtype, tiles):
    """The ghost window of the fused kernels (T8gpuPlainPlan.ghost_buf / send_map: what the multi-rank step driver
    attaches to the launches of its ghost-reading tiles): the A tiles read their ghosts from the receive buffer in the wire
    format and write the elements a peer mirrors into the send buffer in their RK epilogue -- no pack kernel after the first
    stage, no unpack kernel, the mirror slots of the planes stay NaN throughout. All ranks of a k-way partition on one GPU,
    the transport a loopback copy; bitwise the single-rank run. 5 and 7 ranks: elements with several send slots (send_list)."""
    import ctypes as C
    from t8gpu_amd import fused, hip
    mesh = SynthMesh(2, 4, 7, band=0.06) if tiles == "small" else SynthMesh(2, 5, 9, band=0.08)
    whole = mesh.partition()
    st = perturbed_state(whole, 78)
    ref = PlainSolver(whole, dtype, mode="fused", state=st)
    parts = [mesh.partition(r, world) for r in range(world)]
    solvers, halos, windows, keep = [], [], [], []
    multi = 0
    for part in parts:
        gidx = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        local = st[:, gidx].copy()
        local[:, part.N:] = np.nan                              # the mirror slots are never filled: nobody may read them
        opts = dict(tmax=32, fcap=80) if tiles == "small" else (dict(compressed=False) if tiles == "generic" else {})
        s = PlainSolver(part, dtype, mode="fused", state=local, plan_options=opts)
        h = HaloExchange(part, dtype, dist=None, overlap=False)
        smap, slist = send_map_of(part.send_idx, part.N)
        multi += int((smap < -1).sum())
        dm, dl = torch.from_numpy(smap).cuda(), torch.from_numpy(slist).cuda()
        w = fused.T8gpuPlainPlan()
        C.pointer(w)[0] = s.plan.c                              # a copy of the plan ...
        w.ghost_buf, w.send_map, w.send_list, w.send_buf, w.n_owned = (h.recvbuf.data_ptr(), dm.data_ptr(), dl.data_ptr(),
                                                                      h.sendbuf.data_ptr(), part.N)   # ... with the window
        solvers.append(s); halos.append(h); windows.append(w); keep.append((dm, dl))
    if tiles == "patches" and world > 2:
        assert sum(s.plan.host.n_patch_class[2] for s in solvers) > 0      # patch tiles among the ghost-reading ones
    if world > 2:
        assert multi > 0                                                    # elements with more than one send slot
    dt = 0.1 * 2.0 ** -mesh.finest_level
    mirrors = [s.planes[:20, p.N:p.N + p.G].clone() for s, p in zip(solvers, parts)]
    for step in range(3):
        ref.iterate(dt)
        for s in solvers:
            s.begin_step()
        for k in range(3):
            if step == 0 and k == 0:                                        # the state came from outside: pack once
                for s, h in zip(solvers, halos):
                    h._pack(s.step_planes(s.stage_steps(k)[0]))
            loopback(halos)                                                 # (reads every send buffer before anyone rewrites it)
            torch.cuda.synchronize()
            for s, w in zip(solvers, windows):
                src, dst = s.stage_steps(k)
                ni, nt = s.plan.host.n_interior, s.plan.host.ntiles
                args = (s.get_own_variables(s.prev), s.get_own_variables(src), s.get_own_variables(dst), hip.ptr(s.planes[25]),
                        hip.fscalar(dtype, dt), hip.ptr(s.speed) if k == 2 else None, hip.stream_ptr())
                hip.call("t8gpu_hip_plain_fused_stage", dtype, s.kind, k + 1, C.byref(s.plan.c), 0, ni, *args)
                hip.call("t8gpu_hip_plain_fused_stage", dtype, s.kind, k + 1, C.byref(w), ni, nt - ni, *args)
            torch.cuda.synchronize()
    full = torch.cat([s.state() for s in solvers], dim=1).cpu().numpy()
    assert not np.isnan(full).any()
    assert np.array_equal(full, ref.state().cpu().numpy())
    for s, part, m in zip(solvers, parts, mirrors):                         # the mirror slots were never written
        assert torch.allclose(s.planes[:20, part.N:part.N + part.G], m, rtol=0, atol=0, equal_nan=True)
    assert torch.equal(torch.cat([s.speed[:p.F] for s, p in zip(solvers, parts) if p.F]).isfinite().all(), torch.tensor(True, device="cuda"))


def test_pack_unpack_kernels_match_numpy():
    mesh = SynthMesh(2, 4, 6, band=0.06)
    part = mesh.partition(1, 3)
    h = HaloExchange(part, torch.float64, dist=None, overlap=False)
    tot = part.N + part.G
    planes = torch.arange(5 * tot, dtype=torch.float64, device="cuda").reshape(5, tot).contiguous()
    h._pack(planes)
    want = planes[:, torch.from_numpy(part.send_idx).long().cuda()].t().reshape(-1)
    assert torch.equal(h.sendbuf[:5 * h.n_send], want)
    h.recvbuf[:5 * part.G] = torch.arange(5 * part.G, dtype=torch.float64, device="cuda") + 0.5
    before = planes.clone()
    h._unpack(planes)
    assert torch.equal(planes[:, :part.N], before[:, :part.N])
    assert torch.equal(planes[:, part.N:], h.recvbuf[:5 * part.G].view(part.G, 5).t())


@pytest.mark.parametrize("world", [2, 5])
@pytest.mark.parametrize("mode", ["fused", "compat"])
@pytest.mark.parametrize("dim", [3, 2])
def test_k_way_subgrid_partition_on_one_gpu_equals_single_rank(world, mode, dim):
    """Ghost BLOCKS (all 16 / 64 subcells mirrored), interior / ghost-touching block split of the fused kernel."""
    k_way_subgrid(SynthMesh(dim, 3, 4 if dim == 3 else 6, band=0.03), world, mode, dim, both_classes=True)


@pytest.mark.parametrize("mode", ["fused", "compat"])
def test_more_ranks_than_blocks(mode):
    """8 blocks of Subgrid<4,4,4> on 10 ranks: two ranks own nothing."""
    mesh = SynthMesh(3, 1, 1)
    assert sorted(mesh.partition(r, 10, subgrid=True).N for r in range(10)) == [0, 0] + [1] * 8
    k_way_subgrid(mesh, 10, mode, 3, both_classes=False)


def k_way_subgrid(mesh, world, mode, dim, both_classes):
    whole = mesh.partition(subgrid=True)
    S = 4 ** dim
    st = perturbed_state(whole, 78)
    dtype = torch.float64
    ref = SubgridSolver(whole, dtype, mode=mode, state=st)
    parts = [mesh.partition(r, world, subgrid=True) for r in range(world)]
    solvers, halos = [], []
    for part in parts:
        blocks = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        cells = (blocks[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        local = st[:, cells].copy()
        local[:, part.N * S:] = np.nan
        solvers.append(SubgridSolver(part, dtype, mode=mode, state=local))
        halos.append(HaloExchange(part, dtype, dist=None, overlap=False))
    if mode == "fused" and both_classes:
        assert all(0 < s.plan.host.n_interior < s.N for s in solvers)
    dt = 0.1 * 2.0 ** -(mesh.finest_level + 2)
    for _ in range(2):
        ref.iterate(dt)
        for s in solvers:
            s.begin_step()
        for k in range(3):
            for s, h in zip(solvers, halos):
                h._pack(s.step_planes(s.stage_steps(k)[0]))
            loopback(halos)
            for s, h in zip(solvers, halos):
                h._unpack(s.step_planes(s.stage_steps(k)[0]))
            for s in solvers:
                s.run_stage(k, dt, split=True)
    torch.cuda.synchronize()
    full = torch.cat([s.state() for s in solvers], dim=1).cpu().numpy()
    assert not np.isnan(full).any()
    assert rel_err(full, ref.state().cpu().numpy()) < 1e-13
    if mode == "fused":
        assert np.array_equal(full, ref.state().cpu().numpy())      # same sums in the same order on every rank


@pytest.mark.parametrize("dtype,caps,classes", [(torch.float64, (64, 160), 3), (torch.float64, (64, 160), 2), (torch.float32, (64, 160), 2),
                                                (torch.float64, (8, 30), 2), (torch.float32, (8, 30), 3), (torch.float64, (256, 512), 2),
                                                (torch.float64, (256, 512), 3), (torch.float64, (4000, 512), 3)])
def test_native_stepper_with_rccl_self_exchange_on_a_symmetric_problem(dtype, caps, classes):
    """The C++ step driver with its RCCL exchange and two lanes, with REAL data dependencies, on one
    GPU: the mesh and the state are invariant under y -> y + 1/2, which maps the lower half of the Morton
    curve (rank 0 of 2) onto the upper half (rank 1) in order. What rank 1 would send to rank 0 is then
    exactly what rank 0 sends to rank 1, so rank 0 can exchange with ITSELF through a one-rank RCCL
    communicator and must reproduce the single-rank run on its half. (Not bitwise: the single-rank run
    lists the faces at y = 1/2 and at the periodic seam with opposite orientations, so it is symmetric only up
    to rounding; a ghost that is one stage stale would be off by O(dt) ~ 1e-4, far above the tolerance.)
    classes = 2: the plan a partitioned mesh gets by default (interior | ghost-reading tiles; the two-lane driver launches the
    interior as one persistent grid); 3: with the deep / near-boundary split (B tiles on the comm lane)."""
    import types
    from t8gpu_amd import fused, native
    mesh = SynthMesh(2, 5, 8, band=0.05)
    whole, half = mesh.partition(), mesh.partition(0, 2)
    assert half.N * 2 == whole.N and half.peers.tolist() == [1]
    assert np.array_equal(np.diff(half.send_off), np.diff(half.recv_off))
    x, y = whole.centres[:, 0], whole.centres[:, 1]
    rho = 1.5 + 0.4 * np.sin(4 * np.pi * y) * np.cos(2 * np.pi * x)
    v1, v2 = 0.3 * np.cos(4 * np.pi * y), 0.2 * np.sin(2 * np.pi * x) * np.sin(4 * np.pi * y)
    st = np.stack([rho, rho * v1, rho * v2, 0 * rho, 2.5 / 0.4 + 0.5 * rho * (v1 * v1 + v2 * v2)])
    n2 = whole.N // 2
    assert np.allclose(st[:, :n2], st[:, n2:], atol=1e-14)               # the symmetry the test relies on
    st[:, n2:] = st[:, :n2]                                               # ... made exact
    ref = PlainSolver(whole, dtype, mode="fused", state=st)
    gidx = np.concatenate([np.arange(half.N), half.ghost_global])
    local = st[:, gidx].copy()
    local[:, half.N:] = np.nan                                            # ghosts must arrive through RCCL
    g = PlainSolver(half, dtype, mode="fused", state=local, plan_options=dict(tmax=min(caps[0], 256), fcap=caps[1], two_classes=classes == 2),
                    capacity=half.N + half.G + 4)                        # (four extra ghost slots: see `fake` below)
    if caps[0] == 4000:                                                   # no class information: the driver must cope
        g.plan.c.n_deep_tiles = 0
    hp = g.plan.host
    print("tiles C / B / A:", hp.n_deep, hp.n_interior - hp.n_deep, hp.ntiles - hp.n_interior)
    comm = native.NativeComm(0, 1, lambda b, src: b)
    # a second message to the same "peer": the first three send elements once more, received into three extra ghost slots
    # nobody reads -- two messages per peer inside one RCCL group, and elements with two send slots (the driver's send_list).
    # A third message sends the first element a third time into one more spare slot: a run of send_list longer than two.
    extra = 3
    tails = [half.send_off[-1] + extra, half.send_off[-1] + extra + 1]
    fake = types.SimpleNamespace(N=half.N, G=half.G + extra + 1, cells_per_element=1, peers=np.zeros(3, np.int32),
                                 send_off=np.append(half.send_off, tails).astype(np.int32),
                                 recv_off=np.append(half.recv_off, [half.recv_off[-1] + extra, half.recv_off[-1] + extra + 1]).astype(np.int32),
                                 send_idx=np.concatenate([half.send_idx, half.send_idx[:extra], half.send_idx[:1]]).astype(np.int32))
    nh = native.NativeHalo(fake, dtype, comm)
    g.use_native_stepper(nh)
    dt = 0.1 * 2.0 ** -mesh.finest_level
    if caps == (64, 160) and classes == 3:
        assert 0 < hp.n_deep < hp.n_interior < hp.ntiles                  # all three tile classes are populated
    if classes == 2:
        assert 0 < hp.n_deep == hp.n_interior < hp.ntiles
    for _ in range(6 + 13):
        ref.iterate(dt)
    g.iterate(dt)                                                         # one step per call ...
    g.iterate_steps(3, dt)                                                # ... several in one call (odd count) ...
    g.iterate_steps(2, dt)                                                # ... and an even count
    g.iterate_steps(13, dt)                                               # a longer run in one call
    assert native.stream_wait(torch.cuda.current_stream(), 30.0) == 0
    want, got = ref.state().cpu().numpy(), g.state().cpu().numpy()
    assert np.isfinite(got).all()
    assert rel_err(got, want[:, : half.N]) < (1e-12 if dtype == torch.float64 else 1e-5)
    # both send slots of the doubled elements carry the same values, and they are the elements' final state
    sb = nh.sendbuf.view(-1, 5).cpu().numpy()
    n0 = half.send_idx.size
    assert np.array_equal(sb[n0:n0 + extra], sb[:extra])
    assert np.array_equal(sb[:extra], got[:, half.send_idx[:extra]].T)
    # ... and so does the third slot of the element that is sent three times
    assert sb.shape[0] == n0 + extra + 1
    assert np.array_equal(sb[n0 + extra], sb[0]) and np.array_equal(sb[n0 + extra], sb[n0])
    assert np.array_equal(sb[n0 + extra], got[:, half.send_idx[0]])
    g.stepper = None
    comm.destroy()


@pytest.mark.parametrize("dtype,dim", [(torch.float32, 2), (torch.float64, 2), (torch.float64, 3), (torch.float32, 3)])
def test_native_subgrid_stepper_with_rccl_self_exchange_on_a_symmetric_problem(dtype, dim):
    """The C++ step driver for Subgrid blocks (t8gpu_hip_subgrid_stepper_*: deep / near-boundary / ghost-touching
    blocks on the two lanes, whole ghost blocks over RCCL), with real data dependencies on one GPU: mesh and state
    are invariant under a shift by 1/2 along the last axis, which maps rank 0's half of the Morton curve onto rank
    1's, so rank 0 exchanges with itself through a one-rank RCCL communicator and must reproduce the single-rank
    run on its half (to rounding: a block and its image list their remaining coarse faces in different orders; a ghost
    block that is one stage stale would be off by O(dt) ~ 1e-3)."""
    import types
    from t8gpu_amd import native
    mesh = SynthMesh(dim, 3 if dim == 3 else 5, 4 if dim == 3 else 7, band=0.05)
    whole, half = mesh.partition(subgrid=True), mesh.partition(0, 2, subgrid=True)
    S = 4 ** dim
    assert half.N * 2 == whole.N and half.peers.tolist() == [1]
    assert np.array_equal(np.diff(half.send_off), np.diff(half.recv_off))
    st = whole.kh_initial_state().copy()                                  # [5, N * S]; KH is periodic in x, not under the shift:
    n2 = whole.N // 2 * S
    rng = np.random.default_rng(5)
    st[0, :n2] *= 1 + 0.05 * rng.standard_normal(n2)                      # perturb the lower half ...
    st[4, :n2] += 0.3
    st[:, n2:2 * n2] = st[:, :n2]                                         # ... and make the upper half its image
    ref = SubgridSolver(whole, dtype, mode="fused", state=st)
    blocks = np.concatenate([np.arange(half.N), half.ghost_global])
    cells = (blocks[:, None] * S + np.arange(S)[None, :]).reshape(-1)
    local = st[:, cells].copy()
    local[:, half.N * S:] = np.nan                                        # ghost blocks must arrive through RCCL
    g = SubgridSolver(half, dtype, mode="fused", state=local)
    hp = g.plan.host
    print("blocks deep / near / ghost-touching:", hp.n_deep, hp.n_interior - hp.n_deep, half.N - hp.n_interior)
    assert 0 < hp.n_deep < hp.n_interior < half.N
    comm = native.NativeComm(0, 1, lambda b, src: b)
    fake = types.SimpleNamespace(N=half.N, G=half.G, cells_per_element=S, peers=np.zeros(1, np.int32), send_off=half.send_off,
                                 recv_off=half.recv_off, send_idx=half.send_idx)
    g.use_native_stepper(native.NativeHalo(fake, dtype, comm))
    dt = 0.1 * 2.0 ** -(mesh.finest_level + 2)
    for _ in range(1 + 3 + 2 + 7):
        ref.iterate(dt)
    g.iterate(dt)
    g.iterate_steps(3, dt)
    g.iterate_steps(2, dt)
    g.iterate_steps(7, dt)
    assert native.stream_wait(torch.cuda.current_stream(), 30.0) == 0
    want, got = ref.state().cpu().numpy(), g.state().cpu().numpy()
    assert np.isfinite(got).all()
    # fp64: rounding only. fp32 on this deliberately rough field (5 % cell-to-cell noise) amplifies the last bit over
    # 13 steps, most in 3D; a stale ghost block would still be two orders above the bound
    assert rel_err(got, want[:, : half.N * S]) < (1e-11 if dtype == torch.float64 else (2e-6 if dim == 2 else 1e-4))
    # single rank through the same driver (no halo): bitwise the python-driven stages
    one = SubgridSolver(whole, dtype, mode="fused", state=st)
    one.use_native_stepper()
    one.iterate_steps(13, dt)
    torch.cuda.synchronize()
    assert torch.equal(one.state(), ref.state())
    g.stepper = None
    comm.destroy()


def test_bench_native_bring_up_agreement_logic():
    """bench.bring_up_native_stepper with a stand-in process group: success keeps the C++ driver, a rank that
    votes 0 (here: the all-reduce is made to return 0) sends everybody back to the initial state."""
    import sys
    import types
    from t8gpu_amd import native
    sys.path.insert(0, ".")
    import bench
    mesh = SynthMesh(2, 5, 8, band=0.05)
    half = mesh.partition(0, 2)
    comm = native.NativeComm(0, 1, lambda b, src: b)
    fake = types.SimpleNamespace(N=half.N, G=half.G, cells_per_element=1, peers=np.zeros(1, np.int32), send_off=half.send_off,
                                 recv_off=half.recv_off, send_idx=half.send_idx)
    dt = 0.1 * 2.0 ** -mesh.finest_level

    class Group:
        ReduceOp = types.SimpleNamespace(MIN="min")

        def __init__(self, verdict):
            self.verdict = verdict

        def get_backend(self):
            return "nccl"

        def all_reduce(self, t, op=None):
            t.fill_(min(int(t.item()), self.verdict))

    g = PlainSolver(half, torch.float64, mode="fused")
    st = bench.bring_up_native_stepper(g, native.NativeHalo(fake, torch.float64, comm), dt, half, torch.float64, Group(1), 0)
    assert st is not None and g.stepper is st and bool(torch.isfinite(g.state()).all())
    g2 = PlainSolver(half, torch.float64, mode="fused")
    ic = g2.state().clone()
    nh = native.NativeHalo(fake, torch.float64, native.NativeComm(0, 1, lambda b, src: b))
    st = bench.bring_up_native_stepper(g2, nh, dt, half, torch.float64, Group(0), 0)
    assert st is None and g2.stepper is None and (g2.next, g2.prev) == (0, 3) and torch.equal(g2.state(), ic)
    comm.destroy()


def test_bench_make_native_halo_success_path_with_stand_ins():
    """bench.make_native_halo end to end on one GPU: the symmetric half-domain problem, a stand-in process group
    (one rank, self as the only peer) and a stand-in torch.distributed exchange that delivers the rank's own send
    elements as its ghosts -- exactly what the RCCL self-exchange must then reproduce."""
    import sys
    import types
    from t8gpu_amd.halo import HaloExchange
    sys.path.insert(0, ".")
    import bench
    mesh = SynthMesh(2, 5, 8, band=0.05)
    half = mesh.partition(0, 2)
    selfpart = types.SimpleNamespace(N=half.N, G=half.G, cells_per_element=1, peers=np.zeros(1, np.int32), send_off=half.send_off,
                                     recv_off=half.recv_off, send_idx=half.send_idx, rank=0, nranks=1, subgrid=False)

    class Group:
        ReduceOp = types.SimpleNamespace(MIN="min")

        def get_backend(self):
            return "nccl"

        def all_reduce(self, t, op=None):
            pass

        def broadcast_object_list(self, box, src=0):
            pass

    class SelfExchange:
        def __init__(self):
            self.h = HaloExchange(selfpart, torch.float64, dist=None, overlap=False)

        def exchange(self, planes5):
            self.h._pack(planes5)
            self.h.recvbuf.copy_(self.h.sendbuf)
            self.h._unpack(planes5)

    g = PlainSolver(half, torch.float64, mode="fused")
    before = g.planes[0:5].clone()
    nh = bench.make_native_halo(selfpart, torch.float64, g, SelfExchange(), Group(), 0, 1)
    assert nh is not None
    assert torch.equal(g.planes[0:5], before)                         # the check leaves the state as it found it
    nh.comm.destroy()
