"""The kernels of csrc/attr_head.hip one by one against float64 (tests/attr_ref.py, pinned to torch by tests/test_attr_ref_host.py).

Every buffer a kernel writes is a Buf: 64 sentinel values in front and behind, the body prefilled with the sentinel; the guards
must survive and, where the kernel owns the whole body, no sentinel may remain.  Shapes: the dense kernels hold 16-row tiles
(1, 2, 4 or 8 of them, 128 rows per grid row), 16 columns per forward workgroup, 32 per data-gradient workgroup, 64 rows of W
per weight-gradient workgroup, K steps of 32 per wave (256 per forward workgroup of eight waves), 16-byte loads only when K -- in
the data gradient N -- is a multiple of 4; N <= 4 is the small path.  The bounds come from attr_ref.py; nothing is excluded.
The largest error / bound per kernel is printed at the end of the module (recorded in profiles/attr_classifier.md)."""
import numpy as np
import pytest
import torch

import attr_ref as R
from diagan.ops import attr as A

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -12345.625              # finite, exact in fp32, far from every value of these tests
WORST = {}


class Buf:
    """shape-d fp32 tensor on the device between two guard bands of GUARD sentinels; the body starts as `data` or as sentinel."""

    def __init__(self, shape, data=None):
        self.n = int(np.prod(shape))
        self.full = torch.full((self.n + 2 * GUARD,), SENT, dtype=torch.float32, device='cuda')
        self.t = self.full[GUARD:GUARD + self.n].view(shape)
        if data is not None:
            self.t.copy_(data)

    def host(self, written=True):
        torch.cuda.synchronize()
        full = self.full.cpu()
        assert bool((full[:GUARD] == SENT).all() and (full[GUARD + self.n:] == SENT).all()), "guard band overwritten"
        b = full[GUARD:GUARD + self.n]
        if written:
            assert not bool((b == SENT).any()), "an element was left unwritten"
        return b.view(self.t.shape)


def note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))


def check(kernel, what, got, want, bound):
    """|got - want| <= bound element by element; bound None: bit for bit against the fp32 rounding of want."""
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    got = got.reshape(-1)
    assert got.numel() == want.numel()
    if bound is None:
        wrong = int((got != want.float()).sum())
        assert wrong == 0, (kernel, what, f"{wrong} elements differ from the exact result")
        note(kernel, 0.0)
        return
    bound = torch.as_tensor(bound, dtype=torch.float64).reshape(-1)
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{kernel} {what}: worst error / bound {worst:.3f}")
    note(kernel, worst)
    assert worst <= 1.0 and not bool(got.isnan().any()), (kernel, what, worst, int((ratio > 1).sum()))


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    print("\n| kernel | largest error / bound |\n|---|---|")
    for k in sorted(WORST):
        print(f"| {k} | {WORST[k]:.3f} |")


def randn(shape, seed):
    return torch.randn(shape, generator=R.gen(seed))


def keep_mask(shape, seed, zero_rows=()):
    m = (torch.rand(shape, generator=R.gen(seed)) < 0.5).float()
    for r in zero_rows:
        if r < shape[0]:
            m[r] = 0.0
    return m


# ---- pool + flatten ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 3), (2, 3), (7, 7), (9, 9)])
@pytest.mark.parametrize("C", [4, 20])
@pytest.mark.parametrize("B", [1, 3])
def test_pool_flatten(hw, C, B):
    x = randn((B, hw[0], hw[1], C), 10 + 7 * hw[0] + hw[1] + C + B)
    out = Buf((B, C * 49))
    A.pool_flatten(x.cuda(), out=out.t)
    got = out.host()
    want, bound = R.pool_flatten64(x)
    check("attr_pool_flatten_kernel", f"{hw} C={C} B={B}", got, want, bound)
    if hw == (2, 2):                     # the real workload: bins 0-2 copy pixel 0, bin 3 averages, bins 4-6 copy pixel 1
        g = got.view(B, C, 7, 7)
        nchw = x.permute(0, 3, 1, 2)
        assert torch.equal(g[:, :, 0, 0], nchw[:, :, 0, 0]) and torch.equal(g[:, :, 2, 6], nchw[:, :, 0, 1])
        assert torch.equal(g[:, :, 5, 1], nchw[:, :, 1, 0]) and torch.equal(g[:, :, 6, 4], nchw[:, :, 1, 1])
    if hw == (7, 7):                     # identity bins: the output is the NCHW transpose, which pins the flatten order
        assert torch.equal(got.view(B, C, 7, 7), x.permute(0, 3, 1, 2))


# ---- dense forward ----------------------------------------------------------------------------------------------------------------
# M: 1, a tile - 1, a tile, a tile + 1, the ragged last batch, the full batch, past a grid row; K: one step, a multiple of 4 that
# is no multiple of the step, an odd K (scalar loads), more than one workgroup step; N: the small path, a tile, a tile + 1
FWD_CASES = [(1, 32, 2), (1, 131, 16), (15, 32, 17), (16, 100, 16), (17, 131, 17), (17, 300, 2), (33, 100, 4), (82, 300, 16),
             (82, 131, 2), (128, 32, 17), (128, 300, 16), (128, 260, 2), (130, 100, 17), (65, 516, 33), (3, 5, 5)]


@pytest.mark.parametrize("M,K,N", FWD_CASES)
def test_dense_fwd(M, K, N):
    seed = 100 + M + 3 * K + 5 * N
    x, w, b = randn((M, K), seed), randn((N, K), seed + 1) / K ** 0.5, randn((N,), seed + 2)
    mask = keep_mask((M, N), seed + 3)
    xd, wd, bd, md = x.cuda(), w.cuda(), b.cuda(), mask.cuda()
    for relu in (False, True):
        for use_mask in (False, True):
            out = Buf((M, N))
            A.dense_fwd(xd, wd, bd, relu=relu, mask=md if use_mask else None, drop_scale=2.0 if use_mask else 1.0, out=out.t)
            want, bound = R.dense_fwd64(x, w, b, relu, mask if use_mask else None, 2.0)
            check("attr_dense_small_kernel" if N <= 4 else "attr_dense_fwd_kernel", f"M={M} K={K} N={N} relu={relu} mask={use_mask}",
                  out.host(), want, bound)
    out = Buf((M, N))                    # no bias, and a keep-scale that is not a power of two
    A.dense_fwd(xd, wd, None, relu=True, mask=md, drop_scale=1.0 / 0.7, out=out.t)
    want, bound = R.dense_fwd64(x, w, None, True, mask, float(np.float32(1.0 / 0.7)))
    check("attr_dense_small_kernel" if N <= 4 else "attr_dense_fwd_kernel", f"M={M} K={K} N={N} no bias", out.host(), want, bound)


def test_dense_fwd_rows_do_not_depend_on_the_batch():
    x, w, b = randn((128, 300), 1), randn((40, 300), 2), randn((40,), 3)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    full = A.dense_fwd(xd, wd, bd, relu=True)
    for rows in (slice(0, 1), slice(5, 22), slice(46, 128)):
        assert torch.equal(A.dense_fwd(xd[rows].contiguous(), wd, bd, relu=True), full[rows])
    small = A.dense_fwd(xd, wd[:2].contiguous(), bd[:2].contiguous())
    assert torch.equal(A.dense_fwd(xd[7:9].contiguous(), wd[:2].contiguous(), bd[:2].contiguous()), small[7:9])


# ---- data gradient ----------------------------------------------------------------------------------------------------------------
# dX [M, K] = dZ [M, N] W [N, K]: N is the reduction (steps of 16 per wave), K the 32-column tiles
DGRAD_CASES = [(1, 32, 2), (15, 31, 16), (16, 33, 17), (17, 64, 100), (82, 100, 2), (82, 40, 131), (128, 96, 64), (128, 33, 2),
               (130, 32, 20)]


@pytest.mark.parametrize("M,K,N", DGRAD_CASES)
def test_dense_dgrad(M, K, N):
    seed = 300 + M + 3 * K + 5 * N
    dy, w = randn((M, N), seed), randn((N, K), seed + 1) / N ** 0.5
    y = torch.relu(randn((M, N), seed + 2))                       # half of it exactly 0
    mask = keep_mask((M, N), seed + 3, zero_rows=(0, 5, M - 1))   # whole rows dropped
    for use_y, use_mask in ((False, False), (True, False), (True, True), (False, True)):
        out = Buf((M, K))
        A.dense_dgrad(dy.cuda(), w.cuda(), y=y.cuda() if use_y else None, mask=mask.cuda() if use_mask else None,
                      drop_scale=2.0 if use_mask else 1.0, out=out.t)
        want, bound = R.dense_dgrad64(dy, w, y if use_y else None, mask if use_mask else None, 2.0)
        got = out.host()
        check("attr_dense_dgrad_kernel", f"M={M} K={K} N={N} y={use_y} mask={use_mask}", got, want, bound)
        if use_mask:
            assert not bool(got[0].any()) and not bool(got[M - 1].any())      # a dropped row has no gradient at all


# ---- fused weight gradient + SGD ----------------------------------------------------------------------------------------------------
WGRAD_CASES = [(1, 32, 2), (1, 300, 65), (82, 33, 16), (82, 257, 2), (17, 100, 64), (128, 516, 17), (128, 31, 130)]


@pytest.mark.parametrize("M,K,N", WGRAD_CASES)
def test_dense_wgrad_flag_writes_the_gradient(M, K, N):
    seed = 500 + M + 3 * K + 5 * N
    dy, x = randn((M, N), seed), randn((M, K), seed + 1)
    y, mask = torch.relu(randn((M, N), seed + 2)), keep_mask((M, N), seed + 3, zero_rows=(0,))
    for use in (False, True):
        kw = dict(y=y.cuda(), mask=mask.cuda(), drop_scale=2.0) if use else {}
        g_w, g_b = A.dense_wgrad(dy.cuda(), x.cuda(), **kw)
        (want_w, bound_w), (want_b, bound_b) = R.dense_wgrad64(dy, x, y if use else None, mask if use else None, 2.0)
        check("attr_dense_wgrad_kernel", f"g_w M={M} K={K} N={N} dz={use}", g_w.cpu(), want_w, bound_w)
        check("attr_dense_wgrad_kernel", f"g_b M={M} K={K} N={N} dz={use}", g_b.cpu(), want_b, bound_b)


@pytest.mark.parametrize("M,K,N", [(1, 40, 2), (82, 131, 17), (82, 64, 2), (128, 300, 70)])
@pytest.mark.parametrize("mu", [0.9, 0.0])
def test_dense_wgrad_sgd_three_steps(M, K, N, mu):
    seed = 700 + M + 3 * K + 5 * N
    lr = 0.05
    lr32, mu32 = float(np.float32(lr)), float(np.float32(mu))      # the scalars as the kernel receives them
    w0, b0 = randn((N, K), seed), randn((N,), seed + 1)
    W, Bv, BW, BB = Buf((N, K), w0), Buf((N,), b0), Buf((N, K), torch.zeros(N, K)), Buf((N,), torch.zeros(N))
    ref = {'w': (w0.double(), 0.0), 'b': (b0.double(), 0.0), 'bw': (torch.zeros(N, K, dtype=torch.float64), 0.0),
           'bb': (torch.zeros(N, dtype=torch.float64), 0.0)}
    for step in range(3):
        dy, x = randn((M, N), seed + 10 * step + 2), randn((M, K), seed + 10 * step + 3)
        y, mask = torch.relu(randn((M, N), seed + 10 * step + 4)), keep_mask((M, N), seed + 10 * step + 5)
        A.dense_wgrad_sgd(dy.cuda(), x.cuda(), W.t, Bv.t, BW.t, BB.t, lr, mu, y=y.cuda(), mask=mask.cuda(), drop_scale=2.0)
        (gw, bgw), (gb, bgb) = R.dense_wgrad64(dy, x, y, mask, 2.0)
        ref['w'], ref['bw'] = R.sgd64(ref['w'][0], ref['bw'][0], gw, lr32, mu32, ref['w'][1], ref['bw'][1], bgw)
        ref['b'], ref['bb'] = R.sgd64(ref['b'][0], ref['bb'][0], gb, lr32, mu32, ref['b'][1], ref['bb'][1], bgb)
        for name, buf in (('w', W), ('bw', BW), ('b', Bv), ('bb', BB)):
            check("attr_dense_wgrad_kernel", f"{name} step {step} M={M} K={K} N={N} mu={mu}", buf.host(), ref[name][0], ref[name][1])


def test_dense_wgrad_refuses_a_batch_over_128():
    dy, x = torch.zeros(129, 4, device='cuda'), torch.zeros(129, 8, device='cuda')
    with pytest.raises(RuntimeError, match="batch of 129"):
        A.dense_wgrad(dy, x)


# ---- cross-entropy ----------------------------------------------------------------------------------------------------------------
def ce_logits(M, N, kind, seed):
    if kind == 'randn':
        return 3.0 * randn((M, N), seed)
    if kind == 'wide':                               # +-80: exp overflows fp32 without the subtraction of the maximum
        z = 80.0 * (2.0 * torch.rand((M, N), generator=R.gen(seed)) - 1.0)
        z[0, 0], z[0, N - 1] = 80.0, -80.0
        return z
    z = 3.0 * randn((M, N), seed)                    # 'tie': rows 0 and M - 1 have every entry equal to the row's maximum
    z[0] = z[0].max()
    z[M - 1] = z[M - 1].max()
    return z


@pytest.mark.parametrize("M", [1, 82, 128])
@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("kind", ['randn', 'wide', 'tie'])
def test_cross_entropy(M, N, kind):
    z = ce_logits(M, N, kind, 900 + M + N)
    g = R.gen(901 + M + N)
    for targets in (torch.randint(0, N, (M,), generator=g), torch.zeros(M, dtype=torch.int64), torch.full((M,), N - 1, dtype=torch.int64)):
        loss, correct = A.accumulators('cuda')
        out = Buf((M, N))
        A.cross_entropy(z.cuda(), targets.cuda(), loss, correct, out=out.t)
        want = R.cross_entropy64(z, targets)
        got = out.host()
        check("attr_ce_kernel", f"dlogit M={M} N={N} {kind}", got, *want['dlogit'])
        check("attr_ce_kernel", f"loss M={M} N={N} {kind}", loss.cpu(), want['loss'][0], want['loss'][1])
        assert int(correct.item()) == want['correct']
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(loss).all())
        if kind == 'tie':                            # the first maximum wins: an all-equal row is correct only for target 0
            assert want['correct'] == int((R.first_argmax(z) == targets).sum())
        # a second batch adds to the same accumulators
        z2, t2 = 3.0 * randn((M, N), 902 + M), torch.randint(0, N, (M,), generator=g)
        A.cross_entropy(z2.cuda(), t2.cuda(), loss, correct)
        want2 = R.cross_entropy64(z2, t2)
        total = want['loss'][0] + want2['loss'][0]
        check("attr_ce_kernel", f"accumulated loss M={M} N={N} {kind}", loss.cpu(), total,
              want['loss'][1] + want2['loss'][1] + R.U64 * abs(total))
        assert int(correct.item()) == want['correct'] + want2['correct']


# ---- count ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 100, 256, 300])
@pytest.mark.parametrize("N", [2, 3])
def test_count(M, N):
    z = randn((M, N), 1100 + M + N)
    z[::3] = z[::3, :1]                              # every third row: all entries equal -> class 0
    if M > 4:
        z[4, 1:] = z[4, 0] + 1.0                     # a tie among the later columns above column 0 -> counted
    counter = torch.zeros(1, dtype=torch.int64, device='cuda')
    A.count(z.cuda(), counter)
    assert int(counter.item()) == R.count64(z)
    assert R.count64(z) == int(torch.count_nonzero(torch.argmax(z, dim=1)))
    z2 = randn((M, N), 1101 + M + N)
    A.count(z2.cuda(), counter)
    assert int(counter.item()) == R.count64(z) + R.count64(z2)
    note("attr_count_kernel", 0.0)
