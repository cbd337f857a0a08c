"""GPU: the grouped 3x3 convolution kernels of the ResNeXt backbones (rt_gconv forward / backward-data, rt_gconv_wgrad) against
F.conv2d(..., groups=G) in fp32 on bf16-rounded operands, their refusal of what they do not implement, and the operand refresh
(rt_weight_prep_batched, rt_adamw_mat) of grouped weights [N][9][Cg] with small C."""
import weakref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL_F32 = 2e-5      # fp32-accumulated result vs fp32 CPU reference (summation order only)
TOL_BF16 = 3e-3     # result rounded to bf16 (2^-9 relative per element)


def bf(t):
    return t.bfloat16().float()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel(a, b):
    a = torch.as_tensor(a).detach().float().cpu(); b = torch.as_tensor(b).detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# (B, H, W, stride, dilation): odd sizes, both strides, the dilated layer4 form
GEOMS = [(1, 7, 9, 1, 1), (3, 7, 9, 2, 1), (3, 3, 4, 1, 2), (1, 3, 4, 2, 1)]
CASES = [(cg, g) for cg in (4, 8, 16, 32, 64) for g in (32, 64)]


def _problem(cg, G, B, H, W, s, dl, seed):
    gen = torch.Generator().manual_seed(seed)
    C = cg * G
    x = bf(torch.randn(B, C, H, W, generator=gen)).requires_grad_(True)
    w = bf(torch.randn(C, cg, 3, 3, generator=gen) / (cg * 9) ** 0.5).requires_grad_(True)
    bias = torch.randn(C, generator=gen) * 0.1
    y = F.conv2d(x, w, bias, stride=s, padding=dl, dilation=dl, groups=G)
    return gen, C, x, w, bias, y


@pytest.mark.parametrize("geo", GEOMS, ids=lambda g: "B%dx%dx%d_s%d_d%d" % g)
@pytest.mark.parametrize("cg,G", CASES, ids=lambda v: str(v))
def test_gconv_fwd_dgrad_wgrad(hip, cg, G, geo):
    B, H, W, s, dl = geo
    gen, C, x, w, bias, y = _problem(cg, G, B, H, W, s, dl, seed=cg * 1000 + G + B * 7 + H + s * 3 + dl)
    Ho, Wo = y.shape[-2:]
    geom = (B, H, W, C, Ho, Wo, C, 3, 3, s, dl)
    xg = nhwc(x.detach()).bfloat16().cuda()
    wk = w.detach().permute(0, 2, 3, 1).contiguous().bfloat16().cuda()            # [C][3][3][Cg]
    # forward + bias + ReLU, fp32 and bf16 outputs
    ob, of = hip.gconv(xg, wk, geom=geom, groups=G, bias=bias.cuda(), act=hip.ACT_RELU, out_bf16=True, out_f32=True, dil=dl)
    ref = nhwc(F.relu(y.detach())).reshape(-1, C)
    assert rel(of, ref) < TOL_F32
    assert rel(ob, ref) < TOL_BF16
    # backward-data with the ReLU gate of the tensor whose gradient is produced (here: x itself, rounded)
    dy = bf(torch.randn(y.shape, generator=gen))
    y.backward(dy)
    gate = bf(torch.randn(B, C, H, W, generator=gen))
    geom_t = (B, Ho, Wo, C, H, W, C, 3, 3, s, dl)
    dyg = nhwc(dy).bfloat16().cuda()
    _, dx = hip.gconv(dyg, wk, geom=geom_t, groups=G, transposed=True, gate=nhwc(gate).bfloat16().cuda(),
                      out_bf16=False, out_f32=True, dil=dl)
    ref_dx = nhwc(x.grad * (gate > 0)).reshape(-1, C)
    assert rel(dx, ref_dx) < TOL_F32
    dxb, _ = hip.gconv(dyg, wk, geom=geom_t, groups=G, transposed=True, dil=dl)
    assert rel(dxb, nhwc(x.grad).reshape(-1, C)) < TOL_BF16
    # weight gradient with the FrozenBN scale: overwrite, then accumulate with an explicit split
    scale = torch.rand(C, generator=gen) + 0.5
    ref_dw = w.grad.permute(0, 2, 3, 1) * scale.view(-1, 1, 1, 1)
    dw = torch.full((C, 3, 3, cg), 7.0, device="cuda")                     # garbage: overwrite must not read it
    hip.gconv_wgrad(dyg, xg, dw, geom=geom, groups=G, scale=scale.cuda(), overwrite=True, dil=dl)
    assert rel(dw, ref_dw) < TOL_F32
    hip.gconv_wgrad(dyg, xg, dw, geom=geom, groups=G, scale=scale.cuda(), msplit=3, dil=dl)
    assert rel(dw, 2 * ref_dw) < TOL_F32


class _Owner:
    pass


@pytest.mark.parametrize("cg,G", [(4, 32), (16, 64), (64, 32)], ids=lambda v: str(v))
def test_gconv_wgrad_norm_accumulator_and_bf16_twin(hip, cg, G):
    B, H, W, s, dl = 3, 7, 9, 2, 1
    gen, C, x, w, bias, y = _problem(cg, G, B, H, W, s, dl, seed=cg + G)
    Ho, Wo = y.shape[-2:]
    dy = bf(torch.randn(y.shape, generator=gen))
    geom = (B, H, W, C, Ho, Wo, C, 3, 3, s, dl)
    xg, dyg = nhwc(x.detach()).bfloat16().cuda(), nhwc(dy).bfloat16().cuda()
    dw = (torch.randn(C, 3, 3, cg, generator=gen) * 0.01).cuda()
    before = dw.clone()
    slots = torch.zeros(hip.SQ_SLOTS * hip.SQ_STRIDE, device="cuda")
    twin = torch.zeros(C, 3, 3, cg, dtype=torch.bfloat16, device="cuda")
    owner = _Owner()
    hip._SQACC_MAP[dw.data_ptr()] = (weakref.ref(owner), slots)
    hip._G16_MAP[dw.data_ptr()] = (weakref.ref(owner), twin.data_ptr())
    try:
        hip.gconv_wgrad(dyg, xg, dw, geom=geom, groups=G, msplit=2)            # accumulate
        torch.cuda.synchronize()
        sq = float(slots.double().sum())
        want = float(dw.double().pow(2).sum() - before.double().pow(2).sum())
        assert abs(sq - want) <= 1e-4 * float(dw.double().pow(2).sum()), (sq, want)
        assert torch.equal(twin, dw.bfloat16())
        slots.zero_()
        hip.gconv_wgrad(dyg, xg, dw, geom=geom, groups=G, overwrite=True)       # overwrite: the new values' squared norm
        torch.cuda.synchronize()
        assert abs(float(slots.double().sum()) - float(dw.double().pow(2).sum())) <= 1e-4 * float(dw.double().pow(2).sum())
        assert torch.equal(twin, dw.bfloat16())
    finally:
        hip._SQACC_MAP.pop(dw.data_ptr(), None)
        hip._G16_MAP.pop(dw.data_ptr(), None)


def test_gconv_refuses_what_it_does_not_implement(hip):
    B, H, W, G, cg = 1, 5, 5, 32, 8
    C = G * cg
    x = torch.randn(B * H * W, C, device="cuda").bfloat16()
    wk = torch.randn(C, 3, 3, cg, device="cuda").bfloat16()
    geom = (B, H, W, C, H, W, C, 3, 3, 1, 1)
    res = torch.zeros(B * H * W, C, device="cuda").bfloat16()
    for kw in (dict(res_bf16=res), dict(res_f32=res.float()), dict(preact=res), dict(drop_p=0.1), dict(tile_hint=1),
               dict(acc2_f32=res.float()), dict(act=hip.ACT_GELU)):
        with pytest.raises(RuntimeError, match="RT_ERR"):
            hip.gconv(x, wk, geom=geom, groups=G, **kw)
    # channels per group outside {4, 8, 16, 32, 64}
    for cg_bad, g_bad in ((2, 128), (12, 32), (128, 2)):
        Cb = cg_bad * g_bad
        xb = torch.randn(B * H * W, Cb, device="cuda").bfloat16()
        wb = torch.randn(Cb, 3, 3, cg_bad, device="cuda").bfloat16()
        gb = (B, H, W, Cb, H, W, Cb, 3, 3, 1, 1)
        with pytest.raises(RuntimeError, match="RT_ERR"):
            hip.gconv(xb, wb, geom=gb, groups=g_bad)
        with pytest.raises(RuntimeError, match="RT_ERR"):
            hip.gconv_wgrad(xb, xb, torch.zeros(Cb, 3, 3, cg_bad, device="cuda"), geom=gb, groups=g_bad)
    # dilation at stride 2, 1x1 kernels, a fused bias gradient
    with pytest.raises(RuntimeError, match="RT_ERR"):
        hip.gconv(x, wk, geom=(B, H, W, C, 3, 3, C, 3, 3, 2, 2), groups=G, dil=2)
    with pytest.raises(RuntimeError, match="RT_ERR"):
        hip.gconv(x, wk.reshape(C, 9, cg)[:, :1].contiguous(), geom=(B, H, W, C, H, W, C, 1, 1, 1, 0), groups=G)
    with pytest.raises(RuntimeError, match="RT_ERR"):
        hip.gconv_wgrad(x, x, torch.zeros(C, 3, 3, cg, device="cuda"), geom=geom, groups=G, dbias=torch.zeros(C, device="cuda"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [4, 8, 16, 32, 64])
def test_operand_refresh_of_grouped_weights(hip, C):
    """Grouped weights are refreshed as N = Cout, T = 9, C = Cg with no transposed copy: rt_weight_prep_batched and the
    operand-emitting AdamW pass (rt_adamw_mat) tile every C in 4 .. 64."""
    gen = torch.Generator().manual_seed(C)
    N, T = 96, 9
    src = torch.randn(N, T, C, generator=gen).cuda()
    scale = (torch.rand(N, generator=gen) + 0.5).cuda()
    dst = torch.full((N, T, C), 3.0, device="cuda").bfloat16()
    wp = hip.WeightPrepBatch(torch.device("cuda"))
    wp.add(src, N, T, C, scale=scale, dst=dst, dst_t=None)
    wp.run()
    assert torch.equal(dst, (src * scale.view(-1, 1, 1)).bfloat16())
    # AdamW over a flat buffer holding two such matrices behind a 4-element head: matrix jobs + chunks vs the flat pass
    from reftr_amd.optim import cover_span
    n = N * T * C
    total = 4 + 2 * n
    p = torch.randn(total, generator=gen).cuda(); g = torch.randn(total, generator=gen).cuda()
    m = torch.randn(total, generator=gen).cuda() * 0.1; v = torch.rand(total, generator=gen).cuda() * 0.1
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    ranges = [(0, total, 1e-3, 1e-4)]
    hip.adamw_flat(p2, g, m2, v2, step=3, ranges=ranges)
    dsts = [torch.zeros(N, T, C, device="cuda").bfloat16() for _ in range(2)]
    jobs, tiles, chunks = cover_span([(4, N, T, C), (4 + n, N, T, C)], 0, total)
    rows = [[off, scale.data_ptr(), d.data_ptr(), 0, N_, T_, C_, first] for (off, N_, T_, C_, first), d in zip(jobs, dsts)]
    mat = (torch.tensor(rows, dtype=torch.int64).cuda(), len(rows), tiles)
    chk = (torch.tensor(chunks, dtype=torch.int64).cuda(), len(chunks) // 2)
    hip.adamw_flat(p, g, m, v, step=3, ranges=ranges, mat=mat, chunks=chk)
    torch.cuda.synchronize()
    for a, b in ((p, p2), (m, m2), (v, v2)):          # masters and moments to 1 ulp (the two kernels are compiled separately)
        assert float((a - b).abs().max()) <= 2e-7 * float(b.abs().max())
    for i, d in enumerate(dsts):
        w32 = p[4 + i * n:4 + (i + 1) * n].view(N, T, C)
        assert torch.equal(d, (w32 * scale.view(-1, 1, 1)).bfloat16())
