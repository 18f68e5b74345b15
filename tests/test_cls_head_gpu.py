"""The kernels of csrc/cls_head.hip one by one against float64 (tests/convnet_ref.py, pinned by tests/test_convnet_ref_host.py).

Every buffer a kernel writes is a Buf: 64 sentinel values in front and behind, the body prefilled with the sentinel; the guards must
survive and, where the kernel owns the whole body, no sentinel may remain.  Shapes: HW = 1 and 3 leave most of the forward
workgroup's rows idle, 81 is the 9 x 9 map of the network tests, 1024 the real 32 x 32 one (16 pixel runs of the data gradient);
C = 4 is one channel group (256 rows of lanes), 20 gives 51 rows and idle lanes, 128 is the network's; N = 1, 2, 20 (the scripts')
and 64 (the limit; more logits than a wave pass covers at once).  The bounds come from convnet_ref.py; nothing is excluded.  The
largest error / bound per kernel is printed at the end of the module (recorded in profiles/group_classifier.md)."""
import numpy as np
import pytest
import torch

import convnet_ref as R
from diagan._native import lpips_abi as cnat
from diagan.ops import cls as K

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -12345.625              # finite, exact in fp32, far from every value of these tests
WORST = {}
HWS, CS, NS, BS = (1, 3, 81, 1024), (4, 20, 128), (1, 2, 20, 64), (1, 3)


class Buf:
    """shape-d tensor on the device between two guard bands of GUARD sentinels; the body starts as `data` or as sentinel."""

    def __init__(self, shape, data=None, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.sent = SENT if dtype.is_floating_point else int(SENT)
        self.full = torch.full((self.n + 2 * GUARD,), self.sent, dtype=dtype, device='cuda')
        self.t = self.full[GUARD:GUARD + self.n].view(shape)
        if data is not None:
            self.t.copy_(data)

    def host(self, written=True):
        torch.cuda.synchronize()
        full = self.full.cpu()
        assert bool((full[:GUARD] == self.sent).all() and (full[GUARD + self.n:] == self.sent).all()), "guard band overwritten"
        b = full[GUARD:GUARD + self.n]
        if written:
            assert not bool((b == self.sent).any()), "an element was left unwritten"
        return b.view(self.t.shape)

    def untouched(self):
        assert bool((self.host(written=False) == self.sent).all()), "a buffer the call was not given to write was written"


def note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))


def check(kernel, what, got, pair):
    want, bound = (torch.as_tensor(t, dtype=torch.float64).reshape(-1) for t in pair)
    got = got.reshape(-1)
    assert got.numel() == want.numel()
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


def fwd_inputs(B, HW, C, N):
    """The last row of a batch of three is off everywhere (an all-zero pooled row); channel 0's shift switches it off in every row."""
    g = R.gen(1000 * HW + 10 * C + N)
    x = torch.randn((3, HW, C), generator=g)
    scale, shift = torch.rand(C, generator=g) + 0.5, 0.3 * torch.randn(C, generator=g)
    shift[0] = -100.0
    x[2] = -(x[2].abs() + 1.0 + shift.abs() / scale)
    w, bias = torch.randn((N, C), generator=g) / C ** 0.5, torch.randn(N, generator=g)
    return x[:B].contiguous(), scale, shift, w, bias


def run_fwd(x, scale, shift, w, bias, logits=True, feat=True):
    B, HW, C = x.shape
    N = w.shape[0]
    bufs = {'pooled': Buf((B, C)), 'logits': Buf((B, N)), 'feat': Buf((B, C))}
    dev = [t.cuda() for t in (x, scale, shift, w, bias)]
    cnat.call("diagan_cls_head_fwd", *[cnat.ptr(t) for t in dev], B, HW, C, N, cnat.ptr(bufs['pooled'].t),
              cnat.ptr(bufs['logits'].t) if logits else None, cnat.ptr(bufs['feat'].t) if feat else None, cnat.current_stream())
    return bufs


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("HW", HWS)
def test_head_fwd(HW, C):
    for N in NS:
        rows = {}
        for B in BS:
            x, scale, shift, w, bias = fwd_inputs(B, HW, C, N)
            want = R.head_fwd64(x, scale, shift, w, bias)
            bufs = run_fwd(x, scale, shift, w, bias)
            got = {k: b.host() for k, b in bufs.items()}
            for k in ('pooled', 'logits', 'feat'):
                check("cls_head_fwd_kernel", f"{k} HW={HW} C={C} N={N} B={B}", got[k], want[k])
            assert bool((got['pooled'][:, 0] == 0).all()), "a channel whose shift switches it off must pool to exactly 0"
            if B == 3:
                assert bool((got['pooled'][2] == 0).all()) and bool((got['feat'][2] == 0).all()), "the all-zero row: feat is 0, not NaN"
                assert torch.equal(got['logits'][2], bias), "the all-zero row's logits are the bias"
            rows[B] = got
        for k in ('pooled', 'logits', 'feat'):
            assert torch.equal(rows[1][k][0], rows[3][k][0]), f"{k}: a row's values depend on the batch it is in"
    # NULL outputs leave their buffers alone and do not change the others
    x, scale, shift, w, bias = fwd_inputs(3, HW, C, 20)
    full = {k: b.host() for k, b in run_fwd(x, scale, shift, w, bias).items()}
    for logits, feat in ((False, True), (True, False), (False, False)):
        bufs = run_fwd(x, scale, shift, w, bias, logits=logits, feat=feat)
        for k, on in (('pooled', True), ('logits', logits), ('feat', feat)):
            if on:
                assert torch.equal(bufs[k].host(), full[k])
            else:
                bufs[k].untouched()


def bwd_inputs(B, HW, C, N):
    g = R.gen(77 + 1000 * HW + 10 * C + N)
    return torch.randn((3, N), generator=g)[:B].contiguous() / 3, torch.randn((N, C), generator=g), torch.rand((3, C), generator=g)[:B].contiguous()


def run_bwd(d, w, pooled, HW, g=True, gw=True, gb=True):
    (B, N), C = d.shape, w.shape[1]
    bufs = {'g': Buf((B, HW, C)), 'gw': Buf((N, C)), 'gb': Buf((N,))}
    dev = [t.cuda() for t in (d, w, pooled)]
    cnat.call("diagan_cls_head_bwd", *[cnat.ptr(t) for t in dev], B, HW, C, N, cnat.ptr(bufs['g'].t) if g else None,
              cnat.ptr(bufs['gw'].t) if gw else None, cnat.ptr(bufs['gb'].t) if gb else None, cnat.current_stream())
    return bufs


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("HW", HWS)
def test_head_bwd(HW, C):
    for N in NS:
        for B in BS:
            d, w, pooled = bwd_inputs(B, HW, C, N)
            want = R.head_bwd64(d, w, pooled, HW)
            got = {k: b.host() for k, b in run_bwd(d, w, pooled, HW).items()}
            assert bool((got['g'] == got['g'][:, :1, :]).all()), "g differs between the pixels of an image"
            check("cls_head_g_kernel", f"g HW={HW} C={C} N={N} B={B}", got['g'][:, 0, :], want['g'])
            check("cls_head_wgrad_kernel", f"gw HW={HW} C={C} N={N} B={B}", got['gw'], want['gw'])
            check("cls_head_wgrad_kernel", f"gb HW={HW} C={C} N={N} B={B}", got['gb'], want['gb'])
    d, w, pooled = bwd_inputs(3, HW, C, 20)
    full = {k: b.host() for k, b in run_bwd(d, w, pooled, HW).items()}
    for flags in ((False, True, True), (True, False, False), (True, True, False), (True, False, True), (False, False, True),
                  (False, True, False)):
        bufs = run_bwd(d, w, pooled, HW, *flags)
        for k, on in zip(('g', 'gw', 'gb'), flags):
            if on:
                assert torch.equal(bufs[k].host(), full[k])
            else:
                bufs[k].untouched()


@pytest.mark.parametrize("B", [8, 19, 128])
def test_head_bwd_batches_past_the_eight_rows_in_flight(B):
    """gw's sum over the batch keeps eight rows' loads in flight: one full group, two groups and a tail of three, the scripts' 128."""
    HW, C, N = 3, 20, 20
    g = R.gen(900 + B)
    d, w, pooled = torch.randn((B, N), generator=g) / B, torch.randn((N, C), generator=g), torch.rand((B, C), generator=g)
    want = R.head_bwd64(d, w, pooled, HW)
    got = {k: b.host() for k, b in run_bwd(d, w, pooled, HW).items()}
    assert bool((got['g'] == got['g'][:, :1, :]).all())
    check("cls_head_g_kernel", f"g B={B}", got['g'][:, 0, :], want['g'])
    check("cls_head_wgrad_kernel", f"gw B={B}", got['gw'], want['gw'])
    check("cls_head_wgrad_kernel", f"gb B={B}", got['gb'], want['gb'])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", (1, 64, 65, 300))
def test_histogram(M, N):
    g = R.gen(5 * M + N)
    z = torch.randint(0, 3, (M, N), generator=g).float()            # three values: exact ties in almost every row
    z[0] = 1.0                                                      # a row that ties everywhere: column 0
    want = R.histogram64(z, N)
    assert int(want.sum()) == M
    counts = Buf((N,), torch.zeros(N, dtype=torch.int64), dtype=torch.int64)
    K.histogram(z.cuda(), counts.t)
    assert torch.equal(counts.host(written=False), want)
    z2 = torch.randn((M, N), generator=g)
    K.histogram(z2.cuda(), counts.t)                                 # a second launch adds
    assert torch.equal(counts.host(written=False), want + R.histogram64(z2, N))
    note("cls_histogram_kernel", 0.0)


def test_refusals():
    x = torch.zeros((1, 1, 6), device='cuda')
    v, w, b = torch.zeros(6, device='cuda'), torch.zeros((2, 6), device='cuda'), torch.zeros(2, device='cuda')
    with pytest.raises(RuntimeError, match="diagan_cls_head_fwd"):
        K.head_fwd(x, v, v, w, b)                                    # C = 6 is no multiple of 4
    with pytest.raises(RuntimeError, match="diagan_cls_histogram"):
        cnat.call("diagan_cls_histogram", cnat.ptr(torch.zeros((1, 65), device='cuda')), 1, 65,
                  cnat.ptr(torch.zeros(65, dtype=torch.int64, device='cuda')), cnat.current_stream())
