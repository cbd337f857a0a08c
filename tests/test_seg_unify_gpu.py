"""GroupNorm and RES-head entry points (csrc/rt_norm.hip, csrc/rt_seg.hip): what the host side refuses, and the CEM block's two
kernels against a float64 restatement of the reference module (models/reftr_segmentation.py:16-41)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BADARG, UNSUPPORTED = -1, -2


def _entries(H, buf):
    """(entry point, descriptor class, fields of an accepted call, [(changed fields, return code)]).  Every pointer is `buf` (8 MiB of
    zeros) and every accepted geometry stays far inside it."""
    gn = dict(B=1, HW=4, C=64, G=8, eps=1e-5)
    gn_tok = dict(gn, x=buf, gamma=buf, beta=buf, stats=buf, y_f32=buf, out_rows_per_img=4, partials=buf, chunks=1)
    gn_tok_b = dict(gn, dy=buf, x=buf, gamma=buf, stats=buf, bstats=buf, dx_f32=buf, out_rows_per_img=4)
    nhwc = dict(gn, x=buf, gamma=buf, beta=buf, stats=buf, y_bf16=buf, ldx=64, ldy=64, act=1, partials=buf, partial_blocks=1)
    nhwc_b = dict(gn, dy=buf, x=buf, gamma=buf, beta=buf, stats=buf, bstats=buf, dx_bf16=buf, ldx=64, lddy=64, lddx=64, act=1)
    up = dict(fpn=buf, a_bf16=buf, out_bf16=buf, B=1, H=4, W=4, h=2, w=2, C=64, ldf=64, lda=64, ldo=64)
    up_b = dict(dy=buf, da=buf, dy_bf16=buf, B=1, H=4, W=4, h=2, w=2, C=64, lddy=64, ldda=64, lddyb=64)
    am = dict(B=1, HW=4, E=256, nh=8, ldk=256, k_rows_per_img=4, k_row_off=0, norm=0.1)
    am_f = dict(am, q=buf, k=buf, mask=buf, P=buf)
    am_b = dict(am, q=buf, k=buf, P=buf, dconcat=buf, dq=buf, dk=buf, ld_dconcat=576, concat_col=512)
    cat = dict(src=buf, mem=buf, out_bf16=buf, B=1, HW=4, E=256, nh=8, ldo=576, mem_rows_per_img=4, src_rows_per_img=4)
    ml = dict(pred=buf, target=buf, sums=buf, B=1, h=2, w=2, Ht=4, Wt=4, ldp=1, inv_norm=1.0)
    ml_f = dict(ml, losses=buf)
    ml_b = dict(ml, dpred=buf, g_focal=buf, g_dice=buf, lddp=1, gbuf=buf)
    cem = dict(hs=buf, w3=buf, b3=buf, res=buf, w2=buf, b2=buf, u=buf, energy=buf, stats=buf, B=1, HW=4, ld=16, E=256)
    cem_f = dict(cem, loss=buf)
    cem_b = dict(cem, g=buf, dres=buf, dhs=buf, dw3=buf, db3=buf, dw2=buf, lddr=16)
    return [
        ("rt_groupnorm_fwd", H.GroupNormDesc, gn_tok, [
            (dict(x=None), BADARG), (dict(stats=None), BADARG), (dict(G=7), UNSUPPORTED), (dict(C=264, G=33), UNSUPPORTED),
            (dict(C=96), UNSUPPORTED), (dict(C=256, G=2), UNSUPPORTED), (dict(partials=None), BADARG), (dict(chunks=65), BADARG),
            (dict(chunks=0), BADARG)]),
        ("rt_groupnorm_bwd", H.GroupNormBwdDesc, gn_tok_b, [
            (dict(bstats=None), BADARG), (dict(G=7), UNSUPPORTED), (dict(C=264, G=33), UNSUPPORTED), (dict(C=256, G=2), UNSUPPORTED)]),
        ("rt_gn_nhwc_fwd", H.GnNhwcDesc, nhwc, [
            (dict(y_bf16=None), BADARG), (dict(G=7), UNSUPPORTED), (dict(ldx=63), UNSUPPORTED), (dict(ldy=63), UNSUPPORTED),
            (dict(G=32), UNSUPPORTED), (dict(C=128, G=128, ldx=128, ldy=128), UNSUPPORTED), (dict(HW=0), UNSUPPORTED),
            (dict(B=0), UNSUPPORTED), (dict(partials=None), BADARG), (dict(HW=65), BADARG)]),            # HW = 65: two pixel blocks, room for one
        ("rt_gn_nhwc_bwd", H.GnNhwcBwdDesc, nhwc_b, [
            (dict(dx_bf16=None), BADARG), (dict(G=7), UNSUPPORTED), (dict(lddy=63), UNSUPPORTED), (dict(lddx=63), UNSUPPORTED),
            (dict(C=128, G=128, ldx=128, lddy=128, lddx=128), UNSUPPORTED), (dict(C=4104, ldx=4104, lddy=4104, lddx=4104), UNSUPPORTED)]),
        ("rt_upsample_add", H.UpsampleAddDesc, up, [
            (dict(fpn=None), BADARG), (dict(ldo=63), UNSUPPORTED), (dict(lda=63), UNSUPPORTED), (dict(h=0), UNSUPPORTED),
            (dict(H=1), UNSUPPORTED), (dict(C=0), UNSUPPORTED)]),
        ("rt_upsample_add_bwd", H.UpsampleAddBwdDesc, up_b, [
            (dict(da=None), BADARG), (dict(ldda=63), UNSUPPORTED), (dict(lddy=63), UNSUPPORTED), (dict(lddyb=63), UNSUPPORTED)]),
        ("rt_attn_map_fwd", H.AttnMapDesc, am_f, [
            (dict(mask=None), BADARG), (dict(nh=7), UNSUPPORTED), (dict(HW=0), UNSUPPORTED), (dict(HW=4688), UNSUPPORTED)]),     # 8 * 4688 * 4 > 150000
        ("rt_attn_map_bwd", H.AttnMapBwdDesc, am_b, [
            (dict(dk=None), BADARG), (dict(E=264), UNSUPPORTED), (dict(nh=7), UNSUPPORTED), (dict(HW=4688), UNSUPPORTED)]),
        ("rt_seg_concat", H.SegConcatDesc, cat, [
            (dict(mem=None), BADARG), (dict(ldo=519), UNSUPPORTED), (dict(E=0), UNSUPPORTED)]),
        ("rt_mask_loss", H.MaskLossDesc, ml_f, [
            (dict(sums=None), BADARG), (dict(h=0), UNSUPPORTED), (dict(ldp=0), UNSUPPORTED), (dict(losses=None), BADARG)]),
        ("rt_mask_loss", H.MaskLossDesc, ml_b, [
            (dict(g_dice=None), BADARG), (dict(lddp=0), BADARG), (dict(gbuf=None), BADARG)]),
        ("rt_cem_fwd", H.CemDesc, cem_f, [
            (dict(loss=None), BADARG), (dict(ld=20), BADARG), (dict(ld=8), BADARG), (dict(HW=0), BADARG), (dict(E=128), UNSUPPORTED),
            (dict(E=128, ld=20), BADARG)]),
        ("rt_cem_bwd", H.CemDesc, cem_b, [
            (dict(dw2=None), BADARG), (dict(lddr=18), BADARG), (dict(ld=20), BADARG), (dict(E=128), UNSUPPORTED)]),
    ]


def test_refused_calls(hip):
    """One case per distinct host check of the 12 entry points (10 in rt_seg.hip, rt_mask_loss in both directions, 2 in rt_norm.hip):
    the return code of each, none of which launches anything.  The unchanged descriptor is accepted, which shows that the one changed
    field is what each refusal answers.  That accepted call does launch, with every pointer on the same zero buffer: inputs alias
    outputs and the CEM kernels see zero norms, a state no caller produces; its results mean nothing and are not looked at, only that
    every index stays inside the buffer matters (the geometries are a few hundred elements, the buffer 2 M floats)."""
    buf = torch.zeros(2 << 20, device="cuda")
    stream = hip._stream()
    for name, cls, good, refused in _entries(hip, buf):
        fn = getattr(hip.lib(), name)
        assert fn(None, stream) == BADARG, name
        assert fn(ctypes.byref(hip._desc(cls, **good)), stream) == 0, name
        for change, code in refused:
            assert fn(ctypes.byref(hip._desc(cls, **dict(good, **change))), stream) == code, (name, change)
    torch.cuda.synchronize()


def cem_errors(hip, HW):
    """max |kernel - float64| / max |float64| per quantity of rt_cem_fwd / rt_cem_bwd, B = 2, E = 256, ld = 64.  One query per image, so
    the reference's softmax over the queries (c1) is 1."""
    B, E, ld = 2, 256, 64
    g = torch.Generator().manual_seed(HW)
    hs = (torch.randn(B, E, generator=g)).bfloat16()
    w3, b3 = torch.randn(16, E, generator=g) * 0.1, torch.randn(16, generator=g) * 0.1
    w2, b2 = torch.randn(16, generator=g) * 0.5, torch.randn(1, generator=g) * 0.1
    res = torch.zeros(B * HW, ld); res[:, :16] = torch.randn(B * HW, 16, generator=g).relu(); res = res.bfloat16()
    gl = 0.8
    # float64 restatement of CEM.forward on the kernel's own (bf16-rounded) inputs
    hs64, res64 = hs.double().requires_grad_(True), res[:, :16].double().view(B, HW, 16).requires_grad_(True)
    w3r, b3r, w2r = (t.double().requires_grad_(True) for t in (w3, b3, w2))
    ec = F.softmax(res64 @ w2r + b2.double(), dim=-1)                                                  # [B, HW]
    rec = F.normalize(hs64 @ w3r.t() + b3r, dim=-1)                                                    # [B, 16]
    tsc = torch.clamp((torch.einsum("bc,bpc->bp", rec, F.normalize(res64, dim=-1)) + 1.0) / 2.0, 1e-6, 1.0 - 1e-6)
    energy = (tsc * ec).sum(-1)
    loss = -torch.log(energy + 1e-6).sum() / B
    (gl * loss).backward()
    cu = lambda t: t.cuda()
    lg, saved = hip.cem_fwd(cu(hs), cu(w3), cu(b3), cu(res), cu(w2), cu(b2), B, HW)
    dres = torch.zeros(B * HW, ld, device="cuda")
    dw3, db3, dw2 = torch.zeros(16, E, device="cuda"), torch.zeros(16, device="cuda"), torch.zeros(16, device="cuda")
    dhs = hip.cem_bwd(cu(hs), cu(w3), cu(b3), cu(res), cu(w2), cu(b2), saved, torch.tensor([gl], device="cuda"), dres, dw3, db3, dw2, B, HW)
    assert float(dres[:, 16:].abs().max()) == 0.0

    def err(mine, ref):
        return float((mine.double().cpu() - ref.detach()).abs().max() / ref.detach().abs().max())
    return dict(loss=err(lg[0], loss), energy=err(saved[1], energy), dres=err(dres[:, :16].reshape(B, HW, 16), res64.grad),
                dhs=err(dhs, hs64.grad), dw3=err(dw3, w3r.grad), db3=err(db3, b3r.grad), dw2=err(dw2, w2r.grad))


# measured on the commit before the kernels were unified (max |kernel - float64| / max |float64|), asserted at 1.5 x.  The figures are a
# few fp32 roundings, so the bound is tight by construction: a later change that reorders one of these sums legitimately can exceed it
# without being wrong; then measure again on that change's parent and say so, rather than reading the failure as a broken kernel.
CEM_MEASURED = {
    35: dict(loss=7.5e-8, energy=7.6e-8, dres=5.5e-7, dhs=1.2e-7, dw3=9.7e-8, db3=7.6e-8, dw2=6.2e-7),
    1100: dict(loss=1.4e-7, energy=8.0e-8, dres=3.3e-7, dhs=1.7e-7, dw3=1.8e-7, db3=1.5e-7, dw2=1.7e-6),
}           # (three runs gave the same figures: with B = 2 every atomic target receives two adds, and a + b has one order)


@pytest.mark.parametrize("HW", [35, 1100])        # 35: most of the 1024 threads hold -inf; 1100: a thread takes a second pixel
def test_cem_fwd_bwd_vs_float64(hip, HW):
    e = cem_errors(hip, HW)
    print("cem rel err HW=%d" % HW, " ".join("%s %.3e" % kv for kv in e.items()))
    for k, measured in CEM_MEASURED[HW].items():
        assert e[k] < 1.5 * measured, (k, e[k], measured)
