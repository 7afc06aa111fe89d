"""-m gpu: the flat L1 family driven directly through ctypes -- `emd_l1_loss` (float atomics on a zero-filled scalar), `emd_l1_loss_ws` (granule
table), `emd_abs_mean_backward`, `emd_residual_l1_backward` -- and through their wrappers in emd_amd.model on views.  References, bars and
the sign-of-zero rules: tests/l1_ref.py.

Shapes.  The loss kernels run 1024 lanes of float4 per block and cap the grid at 512 blocks: n = 0, 1, 3, 4, 5 (scalar tail only / one
float4), 4095, 4096, 4097, 2*4096+3 (one block and its edges, two blocks), 512*4096 (the cap reached exactly), 512*4096+4096+7 (a second trip
of the stride loop and a scalar tail).  The two backward kernels run 256 lanes of float4 per block and cap at 8192 blocks: n = 0, 1, 3, 4, 5,
1023, 1024, 1025, 8192*1024 (the cap exactly) and 8192*1024+1024+3, the smallest size that enters their stride loop (34 MB per tensor,
generated on the device).  Every output lies between guard words; inputs are compared bit for bit afterwards."""
import numpy as np
import pytest
import torch

from tests import l1_ref as lr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LOSS_N = (0, 1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 3, 512 * 4096, 512 * 4096 + 4096 + 7)
BWD_N = (0, 1, 3, 4, 5, 1023, 1024, 1025, 8192 * 1024, 8192 * 1024 + 1024 + 3)
NAN_BITS = 0x7FC00000


def l1(path, n, a, b, loss, grad, scratch=None):
    """a, b, loss, grad, scratch: device addresses or None -> return code (synchronised)."""
    from emd_amd import _lib as L
    if path == "ws":
        rc = L.load().emd_l1_loss_ws(n, a, b, loss, grad, scratch, L.stream())
    else:
        rc = L.load().emd_l1_loss(n, a, b, loss, grad, L.stream())
    torch.cuda.synchronize()
    return rc


def rand(n, seed, centre=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(n, device=DEV, generator=g) - centre


def close(got, want):
    return got == want if want == 0.0 else abs(got - want) <= lr.LOSS_REL * abs(want)


@pytest.mark.parametrize("path", ["atomics", "ws"])
@pytest.mark.parametrize("n", LOSS_N)
def test_l1_loss_value_gradient_and_untouched_neighbours(path, n):
    from emd_amd import _lib as L
    a, b = rand(n, 1), rand(n, 2)
    b[::7] = a[::7]                                                    # d == 0 in every seventh element
    a0, b0 = a.clone(), b.clone()
    scratch = torch.zeros(1024, dtype=torch.int32, device=DEV) if path == "ws" else None
    sp = L.ptr(scratch)
    loss, grad = lr.Guarded(1, DEV), lr.Guarded(n, DEV)
    worst = 0.0

    def run(a_t, b_t, with_grad):
        nonlocal worst
        loss.buf[loss.lo] = NAN_BITS                                   # the scalar must be overwritten, not added to
        assert l1(path, n, a_t.data_ptr(), L.ptr(b_t), loss.ptr(), grad.ptr() if with_grad else None, sp) == L.EMD_OK
        assert loss.guards_intact() and grad.guards_intact() and (scratch is None or not bool(scratch.any()))
        got, want = float(loss.t[0]), lr.loss64(a_t, b_t)
        assert close(got, want), (path, n, got, want)
        worst = max(worst, abs(got - want) / want if want else 0.0)
        return got

    run(a, b, True)
    assert lr.same_bits(grad.t, lr.signed(a.double() - b.double(), lr.inv_n32(n) if n else 0.0))
    grad.buf.fill_(lr.GUARD_BITS)
    run(a, b, False)                                                   # grad == NULL: the buffer that was not handed over keeps its pattern
    assert grad.untouched()
    c = a - 0.5
    run(c, None, True)                                                 # b == NULL: mean |a|
    assert lr.same_bits(grad.t, lr.signed(c, lr.inv_n32(n) if n else 0.0))
    assert run(a, a, True) == 0.0 and not bool(grad.buf[grad.lo:grad.lo + n].any())          # a is b: exactly 0.0, +0.0 everywhere
    assert lr.same_bits(a, a0) and lr.same_bits(b, b0)
    print(f"l1_loss[{path}] n={n}: worst relative error of the loss {worst:.2e}")


def test_l1_loss_ws_table_repeats_and_serves_a_small_grid_after_a_large_one():
    from emd_amd import _lib as L
    scratch = torch.zeros(1024, dtype=torch.int32, device=DEV)
    loss, vals = lr.Guarded(1, DEV), {}
    for n in (512 * 4096 + 4096 + 7, 4097, 2 * 4096 + 3, 5):          # 512 blocks, then 2, 3 and 1 on the same table
        a, b = rand(n, 3), rand(n, 4)
        bits = []
        for _ in range(3):
            loss.buf[loss.lo] = NAN_BITS
            assert l1("ws", n, a.data_ptr(), b.data_ptr(), loss.ptr(), None, scratch.data_ptr()) == L.EMD_OK
            assert not bool(scratch.any()) and loss.guards_intact()
            bits.append(int(loss.buf[loss.lo]))
        assert bits[0] == bits[1] == bits[2], (n, bits)
        vals[n] = float(loss.t[0])
        assert close(vals[n], lr.loss64(a, b))
        assert l1("atomics", n, a.data_ptr(), b.data_ptr(), loss.ptr(), None) == L.EMD_OK
        assert abs(float(loss.t[0]) - vals[n]) <= lr.LOSS_REL * vals[n]


def test_l1_loss_refuses_misaligned_pointers_and_writes_nothing():
    from emd_amd import _lib as L
    n = 40
    a, b, grad, loss = lr.Guarded(n + 4, DEV), lr.Guarded(n + 4, DEV), lr.Guarded(n + 4, DEV), lr.Guarded(1, DEV)
    a.t.copy_(rand(n + 4, 5)); b.t.copy_(rand(n + 4, 6))
    scratch = torch.zeros(1028, dtype=torch.int32, device=DEV)
    A, B, Gr, S = a.ptr(), b.ptr(), grad.ptr(), scratch.data_ptr()
    for path in ("atomics", "ws"):
        for what, args in {"a": (A + 4, B, Gr, S), "b": (A, B + 4, Gr, S), "grad": (A, B, Gr + 4, S), "scratch": (A, B, Gr, S + 4),
                           "n < 0": (A, B, Gr, S)}.items():
            if what == "scratch" and path == "atomics":
                continue
            assert l1(path, -1 if what == "n < 0" else n, args[0], args[1], loss.ptr(), args[2], args[3]) == L.EMD_ERR_INVALID, (path, what)
            assert loss.untouched() and grad.untouched() and not bool(scratch.any()), (path, what)
    assert l1("ws", n, None, B, loss.ptr(), Gr, S) == L.EMD_ERR_INVALID and l1("ws", n, A, B, None, Gr, S) == L.EMD_ERR_INVALID
    assert loss.untouched() and grad.untouched()


def residual_inputs(n):
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(n, device=DEV, generator=g)
    x[::5] = 0.0
    x[1::7] = -0.0
    return x


@pytest.mark.parametrize("g0", [0.37, -2.5])
@pytest.mark.parametrize("n", BWD_N)
def test_abs_mean_backward_is_bit_exact(n, g0):
    from emd_amd import _lib as L
    x, g = residual_inputs(n), torch.tensor([g0], device=DEV)
    x0, out = x.clone(), lr.Guarded(n, DEV)
    assert L.load().emd_abs_mean_backward(n, x.data_ptr(), g.data_ptr(), out.ptr(), L.stream()) == L.EMD_OK
    torch.cuda.synchronize()
    assert out.guards_intact() and lr.same_bits(x, x0) and float(g[0]) == float(np.float32(g0))
    if n:
        assert lr.same_bits(out.t, lr.signed(x, lr.factor32(g0, n)))
        assert not bool(out.buf[out.lo:out.lo + n][x == 0].any())                             # +0.0 for x = +0.0 and x = -0.0, whatever g's sign


UPS = ("same", "two", "a_null", "b_null", "both_null")
GS = ("both", "a_null", "b_null", "both_null")


@pytest.mark.parametrize("n", BWD_N)
def test_residual_l1_backward_every_pointer_form_is_bit_exact(n):
    from emd_amd import _lib as L
    xa = residual_inputs(n)
    xb = -0.5 * xa                                                                            # opposite signs: swapped outputs differ
    u1, u2 = rand(n, 11, 0.5), rand(n, 12, 0.5)
    u1[2::9] = -0.0
    ga, gb = torch.tensor([0.37], device=DEV), torch.tensor([-1.25], device=DEV)
    keep = [t.clone() for t in (xa, xb, u1, u2, ga, gb)]
    oa, ob = lr.Guarded(n, DEV), lr.Guarded(n, DEV)
    for up in UPS:
        for gs in GS:
            ua = None if up in ("a_null", "both_null") else u1
            ub = None if up in ("b_null", "both_null") else (u1 if up == "same" else u2)
            fa, fb = (None if gs in ("a_null", "both_null") else 0.37), (None if gs in ("b_null", "both_null") else -1.25)
            oa.buf.fill_(lr.GUARD_BITS); ob.buf.fill_(lr.GUARD_BITS)
            rc = L.load().emd_residual_l1_backward(n, L.ptr(ua), L.ptr(ub), xa.data_ptr(), xb.data_ptr(), None if fa is None else ga.data_ptr(),
                                                   None if fb is None else gb.data_ptr(), oa.ptr(), ob.ptr(), L.stream())
            torch.cuda.synchronize()
            assert rc == L.EMD_OK and oa.guards_intact() and ob.guards_intact(), (up, gs)
            if n:
                assert lr.same_bits(oa.t, lr.backward32(ua, xa, lr.factor32(fa, n))), (n, up, gs, "a")
                assert lr.same_bits(ob.t, lr.backward32(ub, xb, lr.factor32(fb, n))), (n, up, gs, "b")
            else:
                assert oa.untouched() and ob.untouched()
    assert all(lr.same_bits(t, k) for t, k in zip((xa, xb, u1, u2, ga, gb), keep))


def test_backward_kernels_refuse_bad_arguments_and_write_nothing():
    from emd_amd import _lib as L
    lib, n = L.load(), 24
    bufs = [lr.Guarded(n + 4, DEV) for _ in range(6)]                                         # up_a, up_b, x_a, x_b, out_a, out_b
    for k in range(4):
        bufs[k].t.copy_(rand(n + 4, 20 + k, 0.5))
    g = torch.tensor([0.37], device=DEV)
    P = [b.ptr() for b in bufs]

    def pair(n_, p):
        rc = lib.emd_residual_l1_backward(n_, p[0], p[1], p[2], p[3], g.data_ptr(), g.data_ptr(), p[4], p[5], L.stream())
        torch.cuda.synchronize()
        assert bufs[4].untouched() and bufs[5].untouched()
        return rc
    for k in range(6):
        assert pair(n, [p + 4 if j == k else p for j, p in enumerate(P)]) == L.EMD_ERR_INVALID, k
    for k in (2, 3, 4, 5):
        assert pair(n, [None if j == k else p for j, p in enumerate(P)]) == L.EMD_ERR_INVALID, k
    assert pair(-1, P) == L.EMD_ERR_INVALID

    def single(n_, x, gp, out):
        rc = lib.emd_abs_mean_backward(n_, x, gp, out, L.stream())
        torch.cuda.synchronize()
        assert bufs[4].untouched()
        return rc
    for args in ((n, P[2] + 4, g.data_ptr(), P[4]), (n, P[2], g.data_ptr(), P[4] + 4), (-1, P[2], g.data_ptr(), P[4]), (n, None, g.data_ptr(), P[4]),
                 (n, P[2], g.data_ptr(), None), (n, P[2], None, P[4])):
        assert single(*args) == L.EMD_ERR_INVALID, args


# ---- the wrappers of emd_amd.model on views --------------------------------------------------------------------------------------------------

def views():
    """name -> function of a [2, 3, 7, 5] stack: (i) a contiguous slice 420 bytes into its storage, (ii) a transposed and a strided view."""
    return {"offset_slice": lambda s: s[1], "transposed": lambda s: s[0].transpose(0, 2), "strided": lambda s: s[:, :, ::2, 1:4][1]}


def stack(seed):
    return torch.randn(2, 3, 7, 5, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("view", list(views()))
def test_l1_loss_wrapper_on_views(view):
    from emd_amd.model import l1_loss
    cut = views()[view]
    xs, gs = stack(1), stack(2)
    xs.view(-1)[::4] = gs.view(-1)[::4]                                                       # d == 0 in a quarter of the elements
    gt, x = cut(gs), cut(xs).detach().requires_grad_(True)
    assert view != "offset_slice" or (x.is_contiguous() and x.data_ptr() % 16 != 0)
    ref = x.detach().double().requires_grad_(True)
    (ref - gt.double()).abs().mean().backward()
    loss = l1_loss(x, gt)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - lr.loss64(x.detach(), gt)) <= lr.LOSS_REL * lr.loss64(x.detach(), gt)
    assert x.grad.shape == x.shape and x.grad.stride() == ref.grad.stride()
    assert lr.same_bits(x.grad, lr.signed(x.detach().double() - gt.double(), lr.inv_n32(x.numel())))
    torch.testing.assert_close(x.grad.double(), ref.grad, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("view", list(views()))
def test_abs_mean_wrapper_on_views(view):
    from emd_amd.model import abs_mean
    x = views()[view](stack(3)).detach().requires_grad_(True)
    ref = x.detach().double().requires_grad_(True)
    (-2.5 * ref.abs().mean()).backward()
    loss = abs_mean(x)
    (-2.5 * loss).backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - lr.loss64(x.detach())) <= lr.LOSS_REL * lr.loss64(x.detach())
    assert x.grad.shape == x.shape and x.grad.stride() == ref.grad.stride()
    assert lr.same_bits(x.grad, lr.signed(x.detach(), lr.factor32(-2.5, x.numel())))
    torch.testing.assert_close(x.grad.double(), ref.grad, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("view", list(views()))
def test_residual_pair_wrapper_on_views_with_a_sliced_upstream_gradient(view):
    from emd_amd.model import residual_pair_l1
    cut = views()[view]
    xa, xb = cut(stack(4)).detach().requires_grad_(True), cut(stack(5)).detach().requires_grad_(True)
    up_a, up_b = cut(stack(6)), cut(stack(7))                                                 # (iii): the upstream gradients are such views too
    ga, gb = torch.tensor(0.37, device=DEV), torch.tensor(-1.25, device=DEV)
    ra, rb = xa.detach().double().requires_grad_(True), xb.detach().double().requires_grad_(True)
    torch.autograd.backward([ra, rb, ra.abs().mean(), rb.abs().mean()], [up_a.double(), up_b.double(), ga.double(), gb.double()])
    ya, yb, la, lb = residual_pair_l1(xa, xb)
    torch.autograd.backward([ya, yb, la, lb], [up_a, up_b, ga, gb])
    torch.cuda.synchronize()
    assert lr.same_bits(ya, xa.detach()) and lr.same_bits(yb, xb.detach())
    n = xa.numel()
    for x, y_loss, up, g0, r in ((xa, la, up_a, 0.37, ra), (xb, lb, up_b, -1.25, rb)):
        assert abs(float(y_loss.detach()) - lr.loss64(x.detach())) <= lr.LOSS_REL * lr.loss64(x.detach())
        assert x.grad.shape == x.shape and x.grad.stride() == r.grad.stride()
        assert lr.same_bits(x.grad, lr.backward32(up, x.detach(), lr.factor32(g0, n)))
        torch.testing.assert_close(x.grad.double(), r.grad, rtol=1e-6, atol=1e-7)
