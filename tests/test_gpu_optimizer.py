"""GPU tests of the optimizers (csrc/optimizer.hip, masklab_hip/optimizers.py) against tests/optimizer_ref.py.

One step updates every tensor of SIZES together: the sizes either side of a 16-byte vector, of a block's sweep and of a chunk,
a tensor without elements, 300 small ones, and one whose p, g, m, v start 4 bytes into larger, poisoned buffers.

Element bits: p, m, v equal the float32 NumPy evaluation with the device's own scalars, no exception allowed.
fp64 bar: |got - want| <= 1e-6 S against float64 from the same float32 state (about ten float32 roundings; the float32 NumPy
evaluation measures 1.3e-7 / 1.4e-7 / 2.0e-7 of S for p / m / v, the bar is 5 x that).  Largest ratios |got - want| / S
measured on the MI355X over both optimizers and both weight decays (the float32 NumPy evaluation's own, since the bits are
equal): single steps t = 1, 5, 6, 7: p 1.57e-7, m 1.38e-7, v 1.88e-7; the 12-step trajectories, as a share of the summed
bound: p 0.157, m 0.128, v 0.209."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_memory as D
import optimizer_ref as R
from masklab_hip import _lib

pytestmark = pytest.mark.gpu

CHUNK = _lib.OPT_CHUNK
SIZES = [1, 3, 4, 5, 255, 256, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7, 0] + [64] * 300 + [CHUNK + 3]
MIS = len(SIZES) - 1                       # the misaligned tensor: n mod 4 = 3, more than one chunk
LR = 1e-3
CASES = [(kind, wd) for kind in R.KINDS for wd in (0., 0.01)]
BAR = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _upload(arrays, dev, views=(MIS,)):
    """Host arrays -> device tensors; those of `views` start one element into a poisoned buffer two elements longer.
    -> (tensors, {index: buffer})"""
    out, bufs = [], {}
    for i, a in enumerate(arrays):
        if i in views:
            bufs[i] = D.fill_bytes(torch.empty(a.size + 2, dtype=torch.float32, device=dev), D.POISON)
            t = bufs[i][1:a.size + 1]
            t.copy_(torch.from_numpy(a))
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.from_numpy(a).to(dev)
        out.append(t)
    return out, bufs


def _device_step(dev, kind, h, p, g, m, v, iterations, lr=LR, only=None):
    """One step of ops.optimizer_step from the host state -> (p', m', v' as lists of arrays, the device's scalars, iterations after)."""
    from masklab_hip import ops
    idx = list(range(len(p))) if only is None else list(only)
    views = tuple(k for k, i in enumerate(idx) if i == MIS)
    dp, bp = _upload([p[i] for i in idx], dev, views)
    dg, bg = _upload([g[i] for i in idx], dev, views)
    dm, bm = _upload([m[i] for i in idx], dev, views)
    dv, bv = _upload([v[i] for i in idx], dev, views)
    state, scalars = ops.optimizer_state(dev, iterations, lr), ops.optimizer_scalars_buffer(dev)
    ops.optimizer_step(kind, list(zip(dp, dg, dm, dv)), ops.OptimizerTable(), state, scalars, h["beta_1"], h["beta_2"], h["epsilon"],
                       h["decay"], h["weight_decay"], h["init_lr"])
    torch.cuda.synchronize()
    for bufs, role in ((bp, "p"), (bg, "g"), (bm, "m"), (bv, "v")):
        for b in bufs.values():                                          # the bytes either side of a misaligned view
            edge = b.cpu().numpy()[[0, -1]]
            assert D.poison_elements(edge).all(), f"the step wrote outside the `{role}` view: {edge}"
    for a, b in zip(dg, (g[i] for i in idx)):
        assert a.cpu().numpy().tobytes() == b.tobytes(), "the step changed a gradient"
    read = lambda ts: [t.cpu().numpy() for t in ts]
    return read(dp), read(dm), read(dv), ops.optimizer_scalars_read(scalars), int(state[0].item())


_states, _steps = {}, {}


def _state_before(kind, wd, iterations):
    """The float32 state after `iterations` steps of the float32 NumPy evaluation from zero moments (computed once, shared)."""
    key = (kind, wd, iterations)
    if key not in _states:
        h = R.hyper(kind, weight_decay=wd)
        if iterations == 0:
            p = R.case(SIZES, 7)
            _states[key] = (p, [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p])
        else:
            p, m, v = _state_before(kind, wd, iterations - 1)
            s = R.scalars64(kind, iterations - 1, float(np.float32(LR)), h)
            g = R.gradients(SIZES, 7, iterations - 1)
            new = [R.element32(kind, s, *q) for q in zip(p, g, m, v)]
            _states[key] = tuple([n[k] for n in new] for k in range(3))
    return _states[key]


def _step(dev, kind, wd, iterations):
    """The device's step number iterations + 1 from _state_before (run once, shared by the tests). -> dict"""
    key = (kind, wd, iterations)
    if key not in _steps:
        h = R.hyper(kind, weight_decay=wd)
        p, m, v = _state_before(kind, wd, iterations)
        g = R.gradients(SIZES, 7, iterations)
        got = _device_step(dev, kind, h, p, g, m, v, iterations)
        _steps[key] = dict(h=h, p=p, g=g, m=m, v=v, got=got[:3], scalars=got[3], after=got[4])
    return _steps[key]


def _ratios(kind, s64, state, got):
    """max over the elements of |got - want| / S for p, m, v, want = float64 from the same float32 state."""
    worst = [0., 0., 0.]
    for i, (p, g, m, v) in enumerate(zip(*state)):
        if p.size == 0:
            continue
        want, S = R.step64(kind, s64, p, g, m, v), R.magnitudes(kind, s64, p, g, m, v)
        for k in range(3):
            assert np.all(S[k] > 0)
            worst[k] = max(worst[k], float((np.abs(got[k][i] - want[k]) / S[k]).max()))
    return worst


@pytest.mark.parametrize("kind,wd", CASES)
def test_element_bits_equal_the_float32_evaluation_with_the_device_scalars(dev, kind, wd):
    for iterations in (0, 4, 5, 6):                                       # t = 1, 5 (unrectified), 6, 7 (rectified)
        r = _step(dev, kind, wd, iterations)
        sc = r["scalars"]
        assert r["after"] == iterations + 1 and sc.decays == int(wd != 0)
        assert sc.rectified == (1 if kind == "AdamW" else int(iterations >= 5))
        different = 0
        for i, (p, g, m, v) in enumerate(zip(r["p"], r["g"], r["m"], r["v"])):
            assert R.no_subnormals(R.intermediates32(kind, sc, p, g, m, v)), "the inputs were to have no subnormal intermediate"
            want = R.element32(kind, sc, p, g, m, v)
            for k in range(3):
                different += int((r["got"][k][i].view(np.uint32) != want[k].view(np.uint32)).sum())
        print(f"{kind} wd={wd} t={iterations + 1}: {different} of {3 * sum(SIZES)} values differ from the float32 evaluation")
        assert different == 0


@pytest.mark.parametrize("kind,wd", CASES)
def test_single_steps_within_the_fp64_bar(dev, kind, wd):
    for iterations in (0, 4, 5, 6):
        r = _step(dev, kind, wd, iterations)
        s64 = R.scalars64(kind, iterations, float(np.float32(LR)), r["h"])
        worst = _ratios(kind, s64, (r["p"], r["g"], r["m"], r["v"]), r["got"])
        print(f"{kind} wd={wd} t={iterations + 1}: max |got - want| / S  p {worst[0]:.2e}  m {worst[1]:.2e}  v {worst[2]:.2e}")
        assert max(worst) <= BAR, worst


def _class_run(dev, kind, wd, steps, sizes=SIZES, lrs=None, views=(MIS,)):
    """`steps` steps of the optimizer class from zero moments. -> (optimizer, params {name: tensor}, buffers)"""
    from masklab_hip import optimizers
    opt = getattr(optimizers, kind)(lr=LR, weight_decay=wd)
    tensors, bufs = _upload(R.case(sizes, 7), dev, views)
    params = {f"w{i:03d}": t for i, t in enumerate(tensors)}
    for step in range(steps):
        if lrs is not None:
            opt.lr = lrs[step]
        grads = dict(zip(params, _upload(R.gradients(sizes, 7, step), dev, views)[0]))
        opt.apply_gradients(params, grads)
    return opt, params, bufs


@pytest.mark.parametrize("kind,wd", CASES)
def test_trajectory_of_12_steps_within_the_summed_bar(dev, kind, wd):
    from masklab_hip import optimizers
    opt = getattr(optimizers, kind)(lr=LR, weight_decay=wd)
    tensors, _ = _upload(R.case(SIZES, 7), dev)
    params = {f"w{i:03d}": t for i, t in enumerate(tensors)}
    ref = R.Trajectory(kind, R.case(SIZES, 7), lr=float(np.float32(LR)), weight_decay=wd, init_lr=LR)
    bound = [[np.zeros(n) for n in SIZES] for _ in range(3)]
    worst = [0., 0., 0.]
    for step in range(12):
        g = R.gradients(SIZES, 7, step)
        s64 = R.scalars64(kind, step, ref.lr, ref.h)
        for i in range(len(SIZES)):                                      # this step's bound, from the float64 state it starts from
            S = R.magnitudes(kind, s64, ref.p[i], g[i], ref.m[i], ref.v[i])
            for k in range(3):
                bound[k][i] += BAR * S[k]
        ref.step(g)
        opt.apply_gradients(params, dict(zip(params, _upload(g, dev)[0])))
        got = ([t.cpu().numpy() for t in tensors], [opt._m[n].cpu().numpy() for n in params], [opt._v[n].cpu().numpy() for n in params])
        for k, want in enumerate((ref.p, ref.m, ref.v)):
            for i, n in enumerate(SIZES):
                if n:
                    worst[k] = max(worst[k], float((np.abs(got[k][i] - want[i]) / bound[k][i]).max()))
    print(f"{kind} wd={wd}: 12 steps, max |got - want| / summed bound  p {worst[0]:.2e}  m {worst[1]:.2e}  v {worst[2]:.2e}")
    assert opt.iterations == 12 and max(worst) <= 1., worst


@pytest.mark.parametrize("kind", R.KINDS)
def test_scalars_agree_with_the_float64_restatement(dev, kind):
    from masklab_hip import ops
    for decay in (0., 1e-3):
        for wd in (0., 0.01):
            h = R.hyper(kind, decay=decay, weight_decay=wd, lr=LR, init_lr=2.5e-3)
            for t in (1, 5, 6, 1000):
                state, scalars = ops.optimizer_state(dev, t - 1, 3e-3), ops.optimizer_scalars_buffer(dev)
                ops.optimizer_step(kind, [], ops.OptimizerTable(), state, scalars, h["beta_1"], h["beta_2"], h["epsilon"],
                                   h["decay"], h["weight_decay"], h["init_lr"])
                got, want = ops.optimizer_scalars_read(scalars), R.scalars64(kind, t - 1, float(np.float32(3e-3)), h)
                assert int(state[0].item()) == t and float(ops.optimizer_state_lr(state).item()) == float(np.float32(3e-3))
                assert (got.rectified, got.decays) == (want["rectified"], want["decays"]), (t, decay, wd)
                for f in R.FLOAT_FIELDS:
                    assert abs(getattr(got, f) - want[f]) <= 1e-6 * abs(want[f]), (f, t, decay, wd, getattr(got, f), want[f])
    assert R.scalars64("RectifiedAdam", 4, LR, R.hyper("RectifiedAdam"))["rectified"] == 0


def test_two_runs_give_the_same_bits_and_all_tensors_together_equal_each_alone(dev):
    kind, wd, iterations = "RectifiedAdam", 0.01, 6
    r = _step(dev, kind, wd, iterations)
    again = _device_step(dev, kind, r["h"], r["p"], r["g"], r["m"], r["v"], iterations)
    D.assert_same_bits(list(again[:3]), list(r["got"]), "second run")
    for i in range(len(SIZES)):
        alone = _device_step(dev, kind, r["h"], r["p"], r["g"], r["m"], r["v"], iterations, only=[i])
        D.assert_same_bits([a[0] for a in alone[:3]], [a[i] for a in r["got"]], f"tensor {i} alone")


@pytest.mark.parametrize("kind", R.KINDS)
def test_non_trainable_names_keep_their_bits(dev, kind):
    sizes = SIZES[:11] + [64] * 5 + [CHUNK + 3]
    views = (len(sizes) - 1,)
    opt, params, _ = _class_run(dev, kind, 0.01, 1, sizes, views=views)
    names = list(params)
    frozen = set(names[1::2])
    keep = D.snapshot({n: (params[n], opt._m[n], opt._v[n]) for n in names})
    grads = dict(zip(names, _upload(R.gradients(sizes, 7, 1), dev, views)[0]))
    uploads = opt._table.uploads
    opt.apply_gradients(params, {n: g for n, g in grads.items() if n not in frozen}, trainable=lambda n: n not in frozen)
    now = D.snapshot({n: (params[n], opt._m[n], opt._v[n]) for n in names})
    assert opt._table.uploads == uploads + 1 and opt.iterations == 2
    for n in names:
        if n in frozen:
            D.assert_same_bits(now[n], keep[n], n)
        elif params[n].numel():
            assert all(not np.array_equal(a, b) for a, b in zip(now[n], keep[n])), n
    # the same set again: the table is not uploaded; a set of names does what the predicate did
    opt.apply_gradients(params, grads, trainable=set(names) - frozen)
    assert opt._table.uploads == uploads + 1 and opt.iterations == 3
    D.assert_same_bits(D.snapshot({n: (params[n], opt._m[n], opt._v[n]) for n in sorted(frozen)}), {n: keep[n] for n in sorted(frozen)},
                       "frozen")
    with pytest.raises(ValueError, match="no gradient"):
        opt.apply_gradients(params, {n: g for n, g in grads.items() if n not in frozen})


@pytest.mark.parametrize("kind", R.KINDS)
def test_captured_step_replays_with_the_lr_and_iterations_of_its_replay(dev, kind):
    """7 replays of ONE captured step, lr moved by CyclicLR in between, against 7 eager steps: the same bits, across the
    t = 5 -> 6 change of RectifiedAdam's branch inside one graph."""
    from masklab_hip import optimizers
    from masklab_hip.callbacks import CyclicLR
    sizes, steps = SIZES[:11] + [64] * 20, 7
    host_g = [R.gradients(sizes, 7, s) for s in range(steps)]

    class Model:
        pass

    def run(graphed):
        model = Model()
        opt = model.optimizer = getattr(optimizers, kind)(lr=LR, weight_decay=0.01)
        clr = CyclicLR(base_lr=1e-4, max_lr=1e-3, step_size=3., mode="triangular2")
        clr.set_model(model)
        tensors, _ = _upload(R.case(sizes, 7), dev, ())
        params = {f"w{i:03d}": t for i, t in enumerate(tensors)}
        static = dict(zip(params, _upload(host_g[0], dev, ())[0]))
        graph = None
        if graphed:
            opt.apply_gradients(params, static)                       # the eager step that uploads the table; then back to the start
            zeros = [np.zeros(n, dtype=np.float32) for n in sizes]
            opt.set_weights([np.int64(0)] + zeros + zeros)
            for t, a in zip(tensors, R.case(sizes, 7)):
                t.copy_(torch.from_numpy(a))
            torch.cuda.synchronize()
            uploads = opt._table.uploads
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.apply_gradients(params, static)
            assert opt._table.uploads == uploads and opt.iterations == 0
        clr.on_train_begin()
        flags = []
        for s in range(steps):
            for t, a in zip(static.values(), host_g[s]):
                t.copy_(torch.from_numpy(a))
            if graphed:
                graph.replay()
            else:
                opt.apply_gradients(params, static)
            flags.append(opt.scalars.rectified)
            clr.on_batch_end(s)
        torch.cuda.synchronize()
        return D.snapshot(dict(p=tensors, w=opt.get_weights(), lr=clr.history["lr"], flags=flags, it=opt.iterations))

    eager, replayed = run(False), run(True)
    assert eager["it"] == 7 and len(set(eager["lr"])) > 3
    assert eager["flags"] == ([1] * 7 if kind == "AdamW" else [0] * 5 + [1] * 2)
    D.assert_same_bits(replayed, eager, "graph replays")


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_run_resumes_from_get_weights(dev, kind):
    from masklab_hip import optimizers
    sizes = SIZES[:11] + [64] * 5
    first, params, _ = _class_run(dev, kind, 0.01, 4, sizes, views=())
    weights = first.get_weights()
    assert int(weights[0]) == 4 and len(weights) == 1 + 2 * len(sizes)
    second = getattr(optimizers, kind)(lr=LR, weight_decay=0.01)
    second.set_weights(weights)
    assert second.iterations == 4
    copies = {n: t.clone() for n, t in params.items()}
    for step in (4, 5, 6):                                              # across the step at which RectifiedAdam starts to rectify
        g = R.gradients(sizes, 7, step)
        first.apply_gradients(params, dict(zip(params, _upload(g, dev, ())[0])))
        second.apply_gradients(copies, dict(zip(copies, _upload(g, dev, ())[0])))
    assert second.iterations == 7
    D.assert_same_bits(D.snapshot((copies, second.get_weights())), D.snapshot((params, first.get_weights())), "resumed")
    with pytest.raises(ValueError):
        second.set_weights(weights[:-2])


def test_a_changed_table_is_refused_during_capture(dev, monkeypatch):
    """A captured step holds the table's address and cannot upload: with other tensors than the last eager step's it is
    refused on the host, before anything is enqueued.  (The capture is only claimed here: nothing is captured.)"""
    opt, params, _ = _class_run(dev, "AdamW", 0., 1, [8, 16], views=())
    before = D.snapshot(params)
    grads = {n: torch.ones_like(t) for n, t in params.items()}
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="eager step"):
        opt.apply_gradients(params, grads, trainable={"w000"})            # one tensor where the eager step had two
    monkeypatch.undo()
    assert opt.iterations == 1
    D.assert_same_bits(D.snapshot(params), before, "refused step")
