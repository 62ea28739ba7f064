"""One refinement stage (Joint2BoneFeature): the token-path and MANO parameter packers, StageOp, and the MANO launch for both hands."""
import ctypes as C

import torch

from .. import _capi
from .common import F32, HALF, _ann, _dt, _packing_arith, _tok_wdt, bn_fold
from .conv import ConvOp


def pack_token_mlp(sd, prefix, keep):
    """nn.Sequential(Conv1d(k=1), BatchNorm1d, ReLU, Conv1d(k=1)) -> dir_token_mlp (k-major weights, folded BN)."""
    w1 = sd[prefix + '.0.weight'][:, :, 0]
    s1, b1 = bn_fold(sd, prefix + '.1', sd[prefix + '.0.bias'])
    t = dict(w1t=w1.t().contiguous().float(), s1=s1, b1=b1,
             w2t=sd[prefix + '.3.weight'][:, :, 0].t().contiguous().float(), b2=sd[prefix + '.3.bias'].float().contiguous())
    keep.append(t)
    return _capi.TokenMlp(*(t[k].data_ptr() for k in ('w1t', 's1', 'b1', 'w2t', 'b2')))


def pack_pgcn(sd, prefix, keep, num_layers=4, weight_dtype=torch.float32):
    """weight_dtype float32: exact fp32 matmuls (reference layout); bfloat16: bf16 matmuls = autocast semantics (W transposed)"""
    arr = (_capi.PgcnLayer * num_layers)()
    for i in range(num_layers):
        p = '%s.gconv_layers.%d' % (prefix, i)
        s, b = bn_fold(sd, p + '.bn')
        W = sd[p + '.gconv.W']
        W = W.float().contiguous() if weight_dtype == torch.float32 else W.detach().transpose(2, 3).contiguous().to(torch.bfloat16)
        t = dict(W=W, e1=sd[p + '.gconv.e_1'].float().reshape(-1).contiguous(),
                 bias=sd[p + '.gconv.bias'].float().contiguous(), s=s, b=b)
        keep.append(t)
        arr[i] = _capi.PgcnLayer(t['W'].data_ptr(), t['e1'].data_ptr(), t['bias'].data_ptr(), s.data_ptr(), b.data_ptr(), 1,
                                 _dt(weight_dtype))
    return arr


def pack_ste(sd, prefix, keep, depth=4, weight_dtype=torch.float32):
    """weight_dtype float32: exact fp32 Linears (k-major weights); bfloat16: bf16 Linears = autocast semantics ([out][in])."""
    def f(k):
        t = sd[prefix + '.' + k].float().contiguous()
        keep.append(t)
        return t.data_ptr()

    def ft(k):
        w = sd[prefix + '.' + k]
        t = w.float().t().contiguous() if weight_dtype == torch.float32 else w.detach().to(torch.bfloat16).contiguous()
        keep.append(t)
        return t.data_ptr()
    P = _capi.SteParams()
    P.weight_dtype = _dt(weight_dtype)
    pe = sd[prefix + '.spatial_pos_embed'].float().reshape(42, 128).contiguous()
    keep.append(pe)
    P.pos_embed = pe.data_ptr()
    for i in range(1, depth):                       # block 0 is never executed (transformer/mixSTE.py:197)
        b = 'STEblocks.%d.' % i
        P.blocks[i - 1] = _capi.SteBlock(f(b + 'norm1.weight'), f(b + 'norm1.bias'), ft(b + 'attn.qkv.weight'),
                                         f(b + 'attn.qkv.bias'), ft(b + 'attn.proj.weight'), f(b + 'attn.proj.bias'),
                                         f(b + 'norm2.weight'), f(b + 'norm2.bias'), ft(b + 'mlp.fc1.weight'),
                                         f(b + 'mlp.fc1.bias'), ft(b + 'mlp.fc2.weight'), f(b + 'mlp.fc2.bias'))
    P.num_blocks = depth - 1
    P.snorm_w, P.snorm_b = f('spatial_norm.weight'), f('spatial_norm.bias')
    P.head_ln_w, P.head_ln_b = f('head.0.weight'), f('head.0.bias')
    P.head_wt, P.head_b = ft('head.1.weight'), f('head.1.bias')
    return P


def _pad_rows(t, width=2336):
    """[K, 2334] -> contiguous [K, 2336] (zero padded): 16-byte aligned rows for the MANO kernel's float4 reads"""
    out = torch.zeros(t.shape[0], width, device=t.device, dtype=torch.float32)
    out[:, :t.shape[1]] = t
    return out


def pack_mano(sd, prefix, side, center_idx, keep):
    f = lambda k: sd[prefix + '.' + k].float()  # noqa: E731
    t = dict(shapedirs_t=_pad_rows(f('th_shapedirs').reshape(2334, 10).t()),
             posedirs_t=_pad_rows(f('th_posedirs').reshape(2334, 135).t()),
             v_template=f('th_v_template').reshape(2334).contiguous(),
             j_template=(f('th_J_regressor').double() @ f('th_v_template').double().reshape(778, 3)).float().contiguous(),
             j_shapedirs=torch.einsum('jv,vck->jck', f('th_J_regressor').double(),
                                      f('th_shapedirs').double()).float().contiguous(),
             weights=f('th_weights').contiguous(), hands_mean=f('th_hands_mean').reshape(45).contiguous(),
             comps=f('th_selected_comps').contiguous())
    keep.append(t)
    return _capi.ManoTables(t['shapedirs_t'].data_ptr(), t['posedirs_t'].data_ptr(), t['v_template'].data_ptr(),
                            t['j_template'].data_ptr(), t['j_shapedirs'].data_ptr(), t['weights'].data_ptr(), t['hands_mean'].data_ptr(),
                            t['comps'].data_ptr(), 0 if side == 'right' else 1,
                            -1 if center_idx is None else int(center_idx), 0)


class StageOp(object):
    """Joint2BoneFeature (models/dir.py:19-174) packed for one pyramid level"""

    def __init__(self, sd, p, S, distance, dtype, root_joint, keep):
        self.S, self.distance, self.dtype = S, float(distance), dtype
        self.img2joint = (_capi.TokenMlp * 2)(pack_token_mlp(sd, p + '.img2joint_left.filters', keep),
                                              pack_token_mlp(sd, p + '.img2joint_right.filters', keep))
        self.pos_emb = (_capi.TokenMlp * 2)(pack_token_mlp(sd, p + '.pos_emb_left', keep),
                                            pack_token_mlp(sd, p + '.pos_emb_right', keep))
        self.gpos = pack_token_mlp(sd, p + '.global_pos_emb', keep)
        self.gcn = (pack_pgcn(sd, p + '.gcn_left', keep, weight_dtype=_tok_wdt(dtype)), pack_pgcn(sd, p + '.gcn_right', keep, weight_dtype=_tok_wdt(dtype)))
        self.ste = pack_ste(sd, p + '.interaction', keep, weight_dtype=_tok_wdt(dtype))
        R = _capi.RegressParams()
        t = dict(wt=torch.cat([sd[p + '.regressor.mano_left.weight'].float().t(),
                               sd[p + '.regressor.mano_right.weight'].float().t()], 1).contiguous(),     # [1408][128]
                 bl=sd[p + '.regressor.mano_left.bias'].float().contiguous(),
                 br=sd[p + '.regressor.mano_right.bias'].float().contiguous(),
                 wo=sd[p + '.regressor.offset.weight'].float().contiguous(),
                 bo=sd[p + '.regressor.offset.bias'].float().contiguous())
        keep.append(t)
        R.mano_wt, R.mano_b[0], R.mano_b[1] = (t[k].data_ptr() for k in ('wt', 'bl', 'br'))
        R.off_w, R.off_b = t['wo'].data_ptr(), t['bo'].data_ptr()
        R.emb = pack_token_mlp(sd, p + '.proj_feat_emb', keep)
        self.reg = R
        self.mano = (pack_mano(sd, p + '.regressor.mano_layer_left', 'left', root_joint, keep),
                     pack_mano(sd, p + '.regressor.mano_layer_right', 'right', root_joint, keep))
        s, h = bn_fold(sd, p + '.fusion.1', sd[p + '.fusion.0.bias'])
        self.fusion0 = ConvOp(sd[p + '.fusion.0.weight'], dtype, pad=1, scale=s, shift=h, relu=True)
        self.bone_fusion = None
        if dtype in HALF or _packing_arith() is not None:
            # factorised bone fusion (dir_bone_fusion_forward): w_g[tap][hb][c][n] = weight[n, hb*64+c, ky, kx]; bf16 mode: rounded to
            # bf16, bf16 matrix cores; f16 arithmetic modes: unrounded fp32 operands (exact_f32 = 1), on the exact fp32 matrix cores until
            # DirEngine.calibrate has measured G (g_scale = 0), in split precision on the f16 matrix cores afterwards
            exact = dtype == torch.float32
            w = sd[p + '.fusion.0.weight'].detach()
            w = w.float() if exact else w.to(dtype).float()                                   # [256, 2560, 3, 3]  (rounded to the 16-bit storage kind)
            s_f, h_f = bn_fold(sd, p + '.fusion.1', sd[p + '.fusion.0.bias'])                   # (fusion0.scale carries the f16x3 prescale)
            t = dict(w_g=w.reshape(256, 40, 64, 9).permute(3, 1, 2, 0).contiguous(), scale=s_f.to(w.device), shift=h_f.to(w.device))
            keep.append(t)
            self.bone_fusion = _capi.BoneFusionParams(t['w_g'].data_ptr(), t['scale'].data_ptr(), t['shift'].data_ptr(), 1 if exact else 2 if dtype == torch.float16 else 0)
        self.fusion3 = ConvOp(sd[p + '.fusion.3.weight'], dtype, shift=sd[p + '.fusion.3.bias'])


def run_mano_pair(tables_lr, para_l, para_r, B, flags=None, mesh_uv=False):
    """MANO + projection for both hands in one launch, straight out of the 64-wide parameter vectors
    (pose = para[:, :51], betas = para[:, 51:61], cam = para[:, 61:64]; models/dir.py:272-280).  flags: optional int32 [2, B],
    set to 1 where the 6D root rotation has det < 0 (the reference asserts there, rot6d.py:50).  mesh_uv: also return pd_mesh_uv
    [B,778,2] per hand (fourth entry), which only the training loss reads."""
    dev = para_l.device
    out = [[torch.empty(B, 778, 3, device=dev, dtype=F32), torch.empty(B, 21, 3, device=dev, dtype=F32),
            torch.empty(B, 21, 2, device=dev, dtype=F32)] for _ in range(2)]
    if mesh_uv:
        for o in out:
            o.append(torch.empty(B, 778, 2, device=dev, dtype=F32))
    P2 = C.c_void_p * 2
    base = (para_l.data_ptr(), para_r.data_ptr())
    tabs = (_capi.ManoTables * 2)(tables_lr[0], tables_lr[1])
    _ann('mano', 2.0 * B * 1.2e6, 2 * B * (64 + 778 * 3 + 21 * 3 + 21 * 2) * 4 + 2 * (145 * 2336 + 2334 + 778 * 16 + 16 * 33 + 45 * 46) * 4,
         'B=%d x 2 hands (rot6d + PCA + blend shapes + LBS + projection)' % B)
    rc = _capi.lib().dir_mano_forward_pair(
        tabs, P2(base[0], base[1]), 64, P2(base[0] + 51 * 4, base[1] + 51 * 4), 64, P2(base[0] + 61 * 4, base[1] + 61 * 4), 64,
        P2(out[0][0].data_ptr(), out[1][0].data_ptr()), P2(out[0][1].data_ptr(), out[1][1].data_ptr()),
        P2(out[0][2].data_ptr(), out[1][2].data_ptr()), P2(out[0][3].data_ptr(), out[1][3].data_ptr()) if mesh_uv else None,
        None if flags is None else P2(flags[0].data_ptr(), flags[1].data_ptr()), B, _capi.stream_ptr())
    _capi.check(rc, 'dir_mano_forward_pair')
    return out
