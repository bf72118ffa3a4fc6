"""The device-side k-means (include/cffm_hip.h ABI 13: cffm_kmeans, vss_cffm_amd.kmeans) on the CPU through the fiber emulator.  The GPU
half, at the full sizes, is tests/test_kmeans_gpu.py and shares the run_*(device) bodies below.

Whole k-means trajectories are chaotic (one point flipping between two near-equidistant centres moves both centres and everything after),
so nothing here compares a trajectory with an oracle trajectory.  Every Lloyd step is checked against its definition in fp64 instead:

1. assignment: every point satisfies  D[i, label_i] - min_j D[i, j] <= 2^-14 (|x_i|^2 + |c_label_i|^2)  with fp64 squared distances D
   (the three-pass bf16 split leaves ~2^-16 per product; single-pass bf16, 2^-9, or f16 operands break the bound);
2. update: counts == bincount(labels); a non-empty centre equals the fp64 mean of the points carrying its label within 2e-6 max|x|
   (a two-piece hi + lo split of x would sit at 2^-17 = 7.6e-6 and fail); an empty cluster's centre comes back bit-equal;
3. chained steps: ten iters = 1 calls, each checked by 1 and 2, equal ONE iters = 10 call bit for bit; two runs are bit-identical; the
   fp64 inertia does not rise over an update and rises over the next assignment by at most the margin of 1 summed over the points.
"""
import ctypes as C
import os
import tempfile

import pytest
import torch

import vss_cffm_amd as V
from tests import emu
from vss_cffm_amd import _lib

MARGIN = 2.0 ** -14
UPDATE_TOL = 2e-6
HEAD_TOL = 1e-3       # tests/test_infer_gpu.py / tests/test_boundary.py: the north-star contract on logits


# ---------------------------------------------------------------------------------------------- inputs
def make_points(kind, n, seed):
    """seeded [n,256] fp32 points: 'normal' iid; 'relu' = relu(mode + 0.5 noise) around 30 random modes (post-ReLU features; a few
    clusters of 100 end up empty); 'tight' = 4 randn centres + 0.05 randn noise around 12 modes (several initial centres fall into the
    same mode: near-ties)"""
    g = torch.Generator().manual_seed(seed)
    if kind == 'normal':
        return torch.randn(n, 256, generator=g)
    if kind == 'relu':
        modes = torch.randn(30, 256, generator=g)
        pick = torch.randint(0, 30, (n,), generator=g)
        return torch.relu(modes[pick] + 0.5 * torch.randn(n, 256, generator=g)).contiguous()
    if kind == 'tight':
        modes = 4.0 * torch.randn(12, 256, generator=g)
        pick = torch.randint(0, 12, (n,), generator=g)
        return (modes[pick] + 0.05 * torch.randn(n, 256, generator=g)).contiguous()
    raise KeyError(kind)


def make_init(x, k, seed):
    g = torch.Generator().manual_seed(seed)
    return x[torch.randperm(x.shape[0], generator=g)[:k]].clone()


# ---------------------------------------------------------------------------------------------- one Lloyd step in fp64
def sq_dist(xd, cd):
    return (xd * xd).sum(1)[:, None] - 2.0 * (xd @ cd.t()) + (cd * cd).sum(1)[None, :]


def inertia(xd, cd, lab):
    return float((xd - cd[lab]).square().sum())


def check_step(x, c_in, c_out, labels, counts, tag):
    """checks 1 and 2 of the module docstring for one iters = 1 call; returns (inertia before the update, after it, the summed margin)"""
    xd, ci, co = x.detach().cpu().double(), c_in.detach().cpu().double(), c_out.detach().cpu().double()
    lab, cnt = labels.cpu().long(), counts.cpu().long()
    k = ci.shape[0]
    assert lab.shape == (xd.shape[0],) and cnt.shape == (k,) and co.shape == ci.shape
    assert int(lab.min()) >= 0 and int(lab.max()) < k
    D = sq_dist(xd, ci)
    excess = D.gather(1, lab[:, None])[:, 0] - D.min(dim=1).values
    bound = MARGIN * ((xd * xd).sum(1) + (ci * ci).sum(1)[lab])
    worst = float((excess / bound).max())
    differ = float((lab != D.argmin(dim=1)).double().mean())
    assert torch.equal(cnt, torch.bincount(lab, minlength=k))
    mean = torch.zeros(k, 256, dtype=torch.float64).index_add_(0, lab, xd) / cnt.clamp(min=1)[:, None].double()
    full = cnt > 0
    err = float((co[full] - mean[full]).abs().max()) / float(xd.abs().max())
    print('%s: worst assignment excess %.3e of |x|^2+|c|^2 (bound %.3e), %.2e of the labels differ from the fp64 argmin; update error '
          '%.3e of max|x| (bound %.1e); %d empty clusters' % (tag, worst * MARGIN, MARGIN, differ, err, UPDATE_TOL, int((~full).sum())))
    assert bool((excess <= bound).all()), (tag, worst)
    assert err <= UPDATE_TOL, (tag, err)
    assert torch.equal(c_out.cpu()[~full], c_in.cpu()[~full])
    assert bool(torch.isfinite(c_out).all())
    return inertia(xd, ci, lab), inertia(xd, co, lab), float(bound.sum())


def run_step(device, kind, n, k, seed=0):
    x = make_points(kind, n, seed).to(device)
    init = make_init(x, k, seed + 1)
    c, lab, cnt = V.kmeans(x, k, iters=1, init=init)
    assert c.dtype == torch.float32 and lab.dtype == torch.int32 and cnt.dtype == torch.int32 and c.device == x.device
    check_step(x, init, c, lab, cnt, '%s N=%d K=%d' % (kind, n, k))


def run_chain(device, kind, n, k, seed=0, steps=10):
    x = make_points(kind, n, seed).to(device)
    init = make_init(x, k, seed + 1)
    c, prev_after = init, None
    for s in range(steps):
        c2, lab, cnt = V.kmeans(x, k, iters=1, init=c)
        before, after, margin = check_step(x, c, c2, lab, cnt, '%s N=%d K=%d step %d' % (kind, n, k, s))
        assert after <= before, (s, before, after)                       # the update does not raise the inertia
        if prev_after is not None:
            assert before <= prev_after + margin, (s, prev_after, before)  # nor does the assignment, beyond its arithmetic
        c, prev_after = c2, after
    whole = V.kmeans(x, k, iters=steps, init=init)
    again = V.kmeans(x, k, iters=steps, init=init)
    for a, b, d in zip(whole, (c, lab, cnt), again):
        assert torch.equal(a, b)
        assert torch.equal(a, d)


def raw_call(lib, x, init, iters, ws, labels, counts):
    n, k = x.shape[0], init.shape[0]
    c = init.clone()
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream) if x.is_cuda else None
    rc = lib.cffm_kmeans(P(x), n, k, iters, P(c), P(labels) if labels is not None else None, P(counts) if counts is not None else None, P(ws), st)
    assert rc == 0, lib.cffm_last_error()
    return c


def run_edges(device, n=1000):
    lib = _lib.get()
    n = n + 7                                                            # not a multiple of the 16-point tile
    for k in (1, 8, 33, 128):
        run_step(device, 'normal', n, k, seed=10 + k)
    run_step(device, 'tight', n, 33, seed=20)
    run_step(device, 'relu', 33, 33, seed=21)                            # N = K
    x = make_points('relu', n, 30).to(device)
    # ---- two bit-equal initial centres j < j': nobody gets j', c_j' comes back unchanged
    init = make_init(x, 33, 31)
    init[20] = init[4]
    c, lab, cnt = V.kmeans(x, 33, iters=1, init=init)
    check_step(x, init, c, lab, cnt, 'duplicate centre')
    assert int(cnt[20]) == 0 and not bool((lab == 20).any()) and torch.equal(c[20], init[20]) and int(cnt[4]) > 0
    # ---- a far-away initial centre attracts nothing and comes back unchanged
    init = make_init(x, 100, 32)
    init[5] = 1.0e3
    c, lab, cnt = V.kmeans(x, 100, iters=2, init=init)
    assert int(cnt[5]) == 0 and torch.equal(c[5], init[5])
    # ---- workspace and outputs pre-filled with NaN / garbage: every element read was written by the same call
    init = make_init(x, 100, 33)
    want = V.kmeans(x, 100, iters=2, init=init)
    ws = torch.full((lib.cffm_kmeans_workspace_bytes(n, 100),), 0xFF, dtype=torch.uint8, device=device)      # fp32 0xFFFFFFFF = NaN
    assert bool(torch.isnan(ws[:ws.numel() // 4 * 4].view(torch.float32)).all())
    labels = torch.full((n,), -(2 ** 31), dtype=torch.int32, device=device)
    counts = torch.full((100,), -(2 ** 31), dtype=torch.int32, device=device)
    c = raw_call(lib, x, init, 2, ws, labels, counts)
    assert bool(torch.isfinite(c).all())
    for a, b in zip(want, (c, labels, counts)):
        assert torch.equal(a, b)
    ws.fill_(0xFF)
    assert torch.equal(raw_call(lib, x, init, 2, ws, None, None), c)      # labels_out / counts_out may be NULL
    assert torch.equal(V.kmeans(x, 100, iters=2, init=init, ws=ws)[0], c)
    # ---- [2,N,256] = two single calls
    x2 = torch.stack([x, make_points('normal', n, 34).to(device)])
    init2 = torch.stack([make_init(x2[0], 8, 35), make_init(x2[1], 8, 36)])
    both = V.kmeans(x2, 8, iters=2, init=init2)
    assert both[0].shape == (2, 8, 256) and both[1].shape == (2, n) and both[2].shape == (2, 8)
    for i in range(2):
        one = V.kmeans(x2[i], 8, iters=2, init=init2[i])
        for a, b in zip(both, one):
            assert torch.equal(a[i], b)
    # ---- init = None draws x[randperm(N)[:k]] per clip, as head._kmeans does
    torch.manual_seed(5)
    drawn = V.kmeans(x, 8, iters=1)
    torch.manual_seed(5)
    init = x[torch.randperm(n, device=x.device)[:8]].clone()
    for a, b in zip(drawn, V.kmeans(x, 8, iters=1, init=init)):
        assert torch.equal(a, b)
    # ---- bad arguments
    for bad in (lambda: V.kmeans(x, 129), lambda: V.kmeans(x, 0), lambda: V.kmeans(x[:20], 33), lambda: V.kmeans(x, 8, iters=0),
                lambda: V.kmeans(x.double(), 8), lambda: V.kmeans(x.t().contiguous().t(), 8), lambda: V.kmeans(x[:, :128].contiguous(), 8)):
        with pytest.raises(_lib.CffmError):
            bad()
    assert lib.cffm_kmeans_workspace_bytes(n, 129) < 0 and lib.cffm_kmeans_workspace_bytes(5, 8) < 0
    assert lib.cffm_kmeans(None, n, 129, 1, None, None, None, None, None) < 0 and b'K=129' in lib.cffm_last_error()


# ---------------------------------------------------------------------------------------------- the prototype-generating head
class CallSpy:
    """counts calls of library entry points through the binding (the pattern of tests/test_infer_gpu.py)"""

    def __init__(self, lib, *names):
        self.lib, self.real, self.n = lib, {k: getattr(lib, k) for k in names}, {k: 0 for k in names}

    def __enter__(self):
        for k, fn in self.real.items():
            def counted(*a, _k=k, _fn=fn):
                self.n[_k] += 1
                return _fn(*a)
            setattr(self.lib, k, counted)
        return self

    def __exit__(self, *exc):
        for k, fn in self.real.items():
            setattr(self.lib, k, fn)


def gene_head(device, seed, **cfg):
    from oracle import recipe as R, ref_import as RI
    from vss_cffm_amd import head as Hd
    from vss_cffm_amd.registry import build_head
    m = build_head(RI.head_cfg(kind='CFFMHead_clips_resize1_8_gene_prototype', **cfg))
    assert not m.load_state_dict(R.synth_state(m, seed=seed), strict=False).unexpected_keys
    m.dropout.p = 0.0
    if device.type == 'cpu':
        Hd.revert_sync_batchnorm(m)               # as tests/test_boundary.py::_my_head does
    return m.to(device).eval()


def run_head(device, feats, k, **cfg):
    from tests import helpers as H
    lib = _lib.get()
    feats = [f.to(device) for f in feats]
    head = gene_head(device, 30, **cfg)
    head.n_clusters = k
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad(), CallSpy(lib, 'cffm_kmeans') as spy:
        metas = [{'filename': tmp + '/data/vid0/origin/0001.jpg'}]
        saved = lambda: torch.load(tmp + '/out/vid0/centers.pt', map_location='cpu')
        head.save_path = tmp + '/out/'
        # ---- the new path: the same logits as the reference's op sequence, one library call, centres in the reference's layout
        torch.manual_seed(11)
        y = head(feats, 1, 4, None, metas)
        assert spy.n['cffm_kmeans'] == 1
        cen = saved()
        assert cen.shape == (1, k, 256) and cen.dtype == torch.float32 and bool(torch.isfinite(cen).all())
        y2 = head.forward_test(feats, metas, None, 1, 4)
        assert spy.n['cffm_kmeans'] == 2 and torch.equal(y, y2)
        # ---- the initial centres are the rows randperm selects for _kmeans: iters = 1 from the same seed through kmeans() itself
        head.kmeans_iters = 1
        torch.manual_seed(12)
        head(feats, 1, 4, None, metas)
        cen1 = saved()
        _, stack, _ = head._rows_front(feats, 1, 4, need_clip=True)
        points = stack.view(-1, 256)
        torch.manual_seed(12)
        init = points[torch.randperm(points.shape[0], device=points.device)[:k]].clone()
        want = V.kmeans(points, k, iters=1, init=init)
        assert torch.equal(cen1[0], want[0].cpu())
        check_step(points, init, want[0], want[1], want[2], 'head points N=%d K=%d' % (points.shape[0], k))
        head.kmeans_iters = 10
        n_calls = spy.n['cffm_kmeans']
        # ---- the fallbacks: the reference's op sequence in torch, no library k-means
        head.rows_impl = 'torch'
        y_ref = head(feats, 1, 4, None, metas)
        assert spy.n['cffm_kmeans'] == n_calls
        e = H.rel_err(y.cpu(), y_ref.cpu())
        print('prototype head, rows path against the torch op sequence: logits rel err %.3e (bound %.0e)' % (e, HEAD_TOL))
        assert y.shape == y_ref.shape and e < HEAD_TOL
        assert saved().shape == (1, k, 256)
        head.rows_impl = 'hip'
        head.n_clusters = 130
        head(feats, 1, 4, None, metas)
        assert spy.n['cffm_kmeans'] == n_calls and saved().shape == (1, 130, 256)
        head.n_clusters = k
        head.train()
        assert head(feats, 1, 4, None, metas) is None                      # (the reference returns nothing in training mode)
        assert spy.n['cffm_kmeans'] == n_calls
        head.eval()
        head(feats, 1, 4, None, metas)
        assert spy.n['cffm_kmeans'] == n_calls + 1


# ---------------------------------------------------------------------------------------------- emulator
@pytest.mark.parametrize('kind,n,k', [('normal', 1999, 100), ('relu', 2000, 100), ('tight', 1200, 100), ('normal', 700, 8)])
def test_one_step_against_the_definition(kind, n, k):
    with emu.active():
        run_step(torch.device('cpu'), kind, n, k)


@pytest.mark.parametrize('kind,n,k', [('relu', 900, 100), ('tight', 600, 33)])
def test_chained_steps_equal_one_call_bit_for_bit(kind, n, k):
    with emu.active():
        run_chain(torch.device('cpu'), kind, n, k)


def test_edges():
    with emu.active():
        run_edges(torch.device('cpu'), n=500)


def test_head_takes_the_rows_path():
    from tests.golden.make_golden_head import feature_maps
    with emu.active():
        run_head(torch.device('cpu'), feature_maps(1, 4, 64), 8)


def test_no_cpu_fallback():
    """a CPU tensor without the emulator raises, GPU present or not (the model: tests/test_abi.py::test_no_cpu_fallback)"""
    with pytest.raises(_lib.CffmError):
        V.kmeans(torch.zeros(64, 256), 8)


def test_abi_13():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cffm_hip.h')).read()
    assert '#define CFFM_ABI_VERSION 13' in text and _lib.ABI_VERSION == 13 and emu.lib().cffm_abi_version() == 13
    assert _lib.SIGNATURES['cffm_kmeans'][1][1] == C.c_long
