"""Execution plan of DIR.forward (eval) on MI355X: parameter packing + the kernel sequence.

Host-side plumbing only: every arithmetic step is a call into libdir_hip.so (include/dir_hip.h).  The plan keeps
feature maps NHWC in the compute dtype (bf16 = BASELINE.json config 2, or fp32 = exact-parity mode), the joint
tokens / MANO path in fp32, folds eval-mode BatchNorm + conv bias into per-channel scale/shift epilogues
(models/backbone/resnet.py:120-140) or prologues (pre-activation hourglass.Residual, models/backbone/hourglass.py:55-70),
lets convs write straight into channel slices of the concat buffers (models/dir.py:444,455,461,470), and launches
on torch's current stream so the whole forward can be captured in a HIP graph (torch.cuda.graph).

State-dict keys are the reference's (963 keys, tests/golden/manifest_dir.json).
"""
import ctypes as C
import os

import torch

from .. import _capi
from .autotune import TunedPlan
from .backbone import BackboneOp
from .common import F32, HALF, _TLS, _ann, _dt, _pow2_scale, bn_fold
from .conv import ConvOp
from .decoder import ConvChainOp, ResidualOp
from .hrnet import HRNetOp
from .stage import StageOp, pack_mano, run_mano_pair


class DirEngine(TunedPlan):
    def __init__(self, state_dict, dtype=torch.bfloat16, root_joint=0, device='cuda', sparse_fusion=True, arith=None):
        """dtype bfloat16: the throughput mode (BASELINE config 2); float32: fp32 feature maps, exact fp32 matrix-core arithmetic
        everywhere (the parity mode of rounds 1-2); float32 with arith='f16x3': the same fp32 feature maps and token path, the
        convolutions on the f16 matrix cores in split precision (3 products per multiply, DIR_DT_F16X3) -- meets the same 1e-4 mm
        budget several times faster."""
        assert dtype in (torch.bfloat16, torch.float16, torch.float32)       # float16: f16 STORAGE (round 5), the bf16 data path with 11-bit significands
        assert arith in (None, 'f16x3', 'f16') and (arith is None or dtype == torch.float32)     # 'f16': one f16 MFMA per product (DIR_DT_F16X1)
        self.arith = arith
        self.tuned_batches = set()
        self._tuned_order = {}                 # batch size -> the conv-family layers in first-call order (autotune / import_tuning)
        self.pending_tuning = None             # {batch size: export_tuning table} handed over by DIR.engine() when the weights were re-packed
        self.sparse_fusion = sparse_fusion     # skip all-zero (tap, bone) K-slabs in the fusion conv (bit-identical)
        _capi.lib()
        self.dtype, self.device = dtype, torch.device(device)
        sd = {k: v.detach().to(self.device) for k, v in state_dict.items()}
        self.keep = []
        _TLS.arith = arith
        try:
            self._pack(sd, root_joint)
        finally:
            _TLS.arith = None

    # ------------------------------------------------------------------------------------------ packing
    def _pack(self, sd, root_joint):
        dt, keep = self.dtype, self.keep
        hr = 'backbone.stage4.0.fuse_layers.0.1.0.weight' in sd              # f4: HRNet-W48 instead of ResNet-50 (no reference counterpart)
        self.bb = HRNetOp(sd, 'backbone', dt, self.device) if hr else BackboneOp(sd, 'backbone', dt, self.device)
        # InitRegressor
        p = 'init_regressor'
        H = _capi.InitHeadParams()
        t = {}
        # both attention branches read c4: ONE 3x3 conv with N = 2 x 1024 (left | right), A operand streamed once
        aw, asc, ash = [], [], []
        for i, side in enumerate(('left', 'right')):
            a = '%s.attention_%s' % (p, side)
            s, h = bn_fold(sd, a + '.1', sd[a + '.0.bias'])
            aw.append(sd[a + '.0.weight']); asc.append(s); ash.append(h)
            t['aw%d' % i] = sd[a + '.3.weight'].float().reshape(-1).contiguous()
            H.attn_w[i] = t['aw%d' % i].data_ptr()
            H.attn_b[i] = float(sd[a + '.3.bias'].float().item())
            t['mb%d' % i] = sd['%s.mano_%s.bias' % (p, side)].float().contiguous()
            H.mano_b[i] = t['mb%d' % i].data_ptr()
        self.attn = ConvOp(torch.cat(aw, 0), dt, pad=1, scale=torch.cat(asc), shift=torch.cat(ash), relu=True)
        t['mwt'] = torch.cat([sd[p + '.mano_left.weight'].float().t(), sd[p + '.mano_right.weight'].float().t()],
                             1).contiguous()                               # [2048][128] k-major
        H.mano_wt = t['mwt'].data_ptr()
        t['ow'], t['ob'] = sd[p + '.offset.weight'].float().contiguous(), sd[p + '.offset.bias'].float().contiguous()
        H.off_w, H.off_b = t['ow'].data_ptr(), t['ob'].data_ptr()
        keep.append(t)
        self.init_head = H
        self.init_mano = (pack_mano(sd, p + '.mano_layer_left', 'left', root_joint, keep),
                          pack_mano(sd, p + '.mano_layer_right', 'right', root_joint, keep))
        # decoder
        d = 'decoder'
        self.res = {k: ResidualOp(sd, '%s.%s' % (d, k), dt) for k in (
            'skip_layer4', 'fusion_layer4', 'enhance_layer4', 'skip_layer3', 'fusion_layer3', 'enhance_layer3')}
        self.stage4 = StageOp(sd, d + '.projecter_4', 16, 1, dt, root_joint, keep)
        self.stage3 = StageOp(sd, d + '.projecter_3', 32, 2, dt, root_joint, keep)
        # f4: further refinement iterations at 32x32 (no reference counterpart; dir_amd.models.dir.FusionJointInterIterDecoder extra_stages)
        self.stages_x, self.res_x = [], []
        while ('%s.projecter_x.%d.fusion.0.weight' % (d, len(self.stages_x))) in sd:
            i = len(self.stages_x)
            self.stages_x.append(StageOp(sd, '%s.projecter_x.%d' % (d, i), 32, 2, dt, root_joint, keep))
            self.res_x.append(ResidualOp(sd, '%s.enhance_layer_x.%d' % (d, i), dt))
        s, h = bn_fold(sd, d + '.conv_final.1')
        self.final0 = ConvOp(sd[d + '.conv_final.0.weight'], dt, pad=1, scale=s, shift=h, relu=True)
        self.final3 = ConvOp(sd[d + '.conv_final.3.weight'], dt, shift=sd[d + '.conv_final.3.bias'])
        # seg / dense heads (models/dir.py:425-433): both read `feat`, so their 3x3 convs run as ONE N = 128 + 128 GEMM and their
        # 1x1 -> 3 convs as one block-diagonal N = 6 GEMM over the 256 merged channels (identical arithmetic per output)
        w0, s0, h0, w3, b3 = [], [], [], torch.zeros(6, 256, 1, 1, device=self.device), []
        for i, k in enumerate(('seg', 'dense')):
            s, h = bn_fold(sd, '%s.%s.1' % (d, k), sd['%s.%s.0.bias' % (d, k)])
            w0.append(sd['%s.%s.0.weight' % (d, k)]); s0.append(s); h0.append(h)
            w3[3 * i:3 * i + 3, 128 * i:128 * i + 128] = sd['%s.%s.3.weight' % (d, k)]
            b3.append(sd['%s.%s.3.bias' % (d, k)])
        self.heads0 = ConvOp(torch.cat(w0, 0), dt, pad=1, scale=torch.cat(s0), shift=torch.cat(h0), relu=True)
        self.heads3 = ConvOp(w3, dt, shift=torch.cat(b3), out_dtype=F32)
        self.final0.link_split(self.final3)
        self.final3.link_split(self.heads0)
        self.heads0.link_split(self.heads3)
        # 16-bit storage: each 3x3 and the 1x1 that alone reads it as one launch (ConvChainOp; the link_split hand-over above is the f16-arithmetic modes')
        self.final_chain = ConvChainOp(self.final0, self.final3)
        self.heads_chain = ConvChainOp(self.heads0, self.heads3)

    # ------------------------------------------------------------------------------------------ pieces
    def init_regressor(self, c4):
        L, dev = _capi.lib(), self.device
        B = c4.shape[0]
        hh = self.attn(c4)                                   # [B,8,8,2048] = (left 1024 | right 1024)
        ch = hh.shape[3] // 2
        esz = hh.element_size()
        para_l = torch.empty(B, 64, device=dev, dtype=F32)
        para_r = torch.empty(B, 64, device=dev, dtype=F32)
        off = torch.empty(B, 3, device=dev, dtype=F32)
        npx = c4.shape[1] * c4.shape[2]
        _ann('init_head', 2.0 * B * (2 * npx * ch + 2 * npx * c4.shape[3] + c4.shape[3] * 128),
             (c4.numel() + hh.numel()) * esz + (c4.shape[3] * 128 + 2 * ch + 131 * 3) * 4 + B * 131 * 4, 'B=%d attention pooling + 3 Linears' % B)
        _capi.check(L.dir_init_head_forward(self.init_head, _capi.ptr(c4), C.c_void_p(hh.data_ptr()),
                                            C.c_void_p(hh.data_ptr() + ch * esz), 2 * ch, _capi.ptr(para_l),
                                            _capi.ptr(para_r), _capi.ptr(off), B, c4.shape[1] * c4.shape[2], c4.shape[3],
                                            ch, _dt(self.dtype), _capi.stream_ptr()), 'dir_init_head_forward')
        return self.mano_outputs(self.init_mano, para_l, para_r, off, self._flags[0] if self._flags is not None else None)

    def mano_outputs(self, tables, para_l, para_r, off, flags=None):
        B = para_l.shape[0]
        (vl, jl, uvl), (vr, jr, uvr) = run_mano_pair(tables, para_l, para_r, B, flags)
        return {'pd_offset': off, 'pd_mano_para_left': para_l, 'pd_mano_para_right': para_r,
                'pd_proj_left': para_l[:, 61:64], 'pd_proj_right': para_r[:, 61:64],
                'pd_mesh_xyz_left': vl, 'pd_mesh_xyz_right': vr, 'pd_joint_xyz_left': jl, 'pd_joint_xyz_right': jr,
                'pd_joint_uv_left': uvl, 'pd_joint_uv_right': uvr, 'pd_rel_joint': None}

    def stage(self, st, feat_buf, feat_cs, prev, img_out, img_coff, want_vis):
        """Joint2BoneFeature.forward.  feat_buf: NHWC buffer whose channels [0,256) are fusion_feat; the stage's
        img_feat is written into img_out[..., img_coff:img_coff+256]."""
        L, dev = _capi.lib(), self.device
        B, S = feat_buf.shape[0], st.S
        sp = _capi.stream_ptr()
        x0 = torch.empty(2, B, 21, 128, device=dev, dtype=F32)
        gp = torch.empty(2, B, 21, 128, device=dev, dtype=F32)
        es = feat_buf.element_size()
        mlp = lambda cin: cin * 128 + 128 * 128          # noqa: E731  (Conv1d cin->128, Conv1d 128->128)
        _ann('grid_tokens', 2.0 * 2 * B * 21 * (mlp(256) + 2 * mlp(3)), 2 * B * 21 * 4 * 256 * es + (2 * mlp(256) + 3 * mlp(3)) * 4 + 4 * B * 21 * 128 * 4,
             'B=%d S=%d bilinear gather + 3 token MLPs, 2 hands' % (B, S))
        _capi.check(L.dir_grid_tokens_forward(
            _capi.ptr(feat_buf), _dt(self.dtype), S, 256, feat_cs, 0, _capi.ptr(prev['pd_joint_uv_left']),
            _capi.ptr(prev['pd_joint_uv_right']), _capi.ptr(prev['pd_joint_xyz_left']),
            _capi.ptr(prev['pd_joint_xyz_right']), _capi.ptr(prev['pd_offset']), st.img2joint, st.pos_emb,
            C.byref(st.gpos), _capi.ptr(x0), _capi.ptr(gp), B, sp), 'dir_grid_tokens_forward')
        tok = torch.empty(B, 42, 128, device=dev, dtype=F32)
        scratch = torch.empty(4, B, 21, 256, device=dev, dtype=F32)
        wes = 2 if self.dtype in HALF else 4
        _ann('pgcn', 2.0 * 4 * 2 * B * 21 * 2 * 128 * 128, 4 * 2 * (2 * 21 * 128 * 128 * wes + 2 * B * 21 * 128 * 4),
             'B=%d 4 layers x 2 hands (per-node W0/W1 %s + neighbour mix + BN + ReLU)' % (B, 'bf16' if wes == 2 else 'f32'))
        _capi.check(L.dir_pgcn_stack_forward_pair(st.gcn[0], st.gcn[1], 4, _capi.ptr(x0), _capi.ptr(gp), _capi.ptr(tok),
                                                  _capi.ptr(scratch), B, sp), 'dir_pgcn_stack_forward_pair')
        y = torch.empty(B, 42, 64, device=dev, dtype=F32)
        blk = 42 * 128 * 384 + 4 * 2 * 42 * 42 * 32 + 42 * 128 * 128 + 2 * 42 * 128 * 256
        _ann('ste', 2.0 * B * (3 * blk + 42 * 128 * 64), B * 42 * (128 + 64) * 4 + (3 * (128 * 384 + 128 * 128 + 2 * 128 * 256) + 128 * 64) * wes,
             'B=%d 42 tokens x 128, 3 blocks + head' % B)
        _capi.check(L.dir_ste_forward(C.byref(st.ste), _capi.ptr(tok), None, _capi.ptr(y), B, sp), 'dir_ste_forward')
        para_l = torch.empty(B, 64, device=dev, dtype=F32)
        para_r = torch.empty(B, 64, device=dev, dtype=F32)
        off = torch.empty(B, 3, device=dev, dtype=F32)
        emb = torch.empty(B, 42, 64, device=dev, dtype=F32)
        _ann('regress', 2.0 * B * (2 * 1408 * 64 + 2691 * 3 + 42 * 2 * 64 * 64), (2 * 1408 * 64 + 2691 * 3 + 2 * 64 * 64) * 4 + B * (42 * 64 * 2 + 2 * 64 * 2 + 6) * 4,
             'B=%d 2 x Linear 1408->64 + Linear 2691->3 + proj_feat_emb' % B)
        _capi.check(L.dir_regress_forward(C.byref(st.reg), _capi.ptr(y), _capi.ptr(prev['pd_mano_para_left']),
                                          _capi.ptr(prev['pd_mano_para_right']), _capi.ptr(prev['pd_offset']),
                                          _capi.ptr(para_l), _capi.ptr(para_r), _capi.ptr(off), _capi.ptr(emb), B, sp),
                    'dir_regress_forward')
        factorised = st.bone_fusion is not None and self.factorised_fusion
        if factorised:
            # bf16 throughput mode: bone_proj + fusion conv as a K = 720 reduction, no [B,S,S,2560] bone map.  The per-sample
            # G tensors need the token features only: they are computed before the MANO layer.
            scratch = torch.empty(L.dir_bone_fusion_scratch_bytes(B), device=dev, dtype=torch.uint8)
            _ann('bone_fusion', 2.0 * B * 9 * 80 * 64 * 256, 9 * 40 * 64 * 256 * 4 + B * 42 * 64 * 4 + B * 9 * 80 * 256 * (4 if self.dtype == F32 else 2),
                 'B=%d G = f_end . W (9 taps x 80 bone ends x 256)' % B)
            _capi.check(L.dir_bone_fusion_prepare(st.bone_fusion, _capi.ptr(emb), _capi.ptr(scratch), B, sp), 'dir_bone_fusion_prepare')
        res = self.mano_outputs(st.mano, para_l, para_r, off, self._flags[self._stage_index(st)] if self._flags is not None else None)
        vis = torch.empty(B, 1280, S, S, device=dev, dtype=F32) if want_vis else None
        if factorised:
            if self.arith is not None and _TLS.calibrating:
                # split-precision fusion (dir_bone_fusion_params.g_scale): the largest |G| of this batch lands in [2^9, 2^10) of the f16 range
                amax = float(scratch.view(F32)[:B * 9 * 40 * 256 * 2].abs().max())
                st.bone_fusion.g_scale = _pow2_scale(amax)
            fused = torch.empty(B, S, S, 256, device=dev, dtype=self.dtype)
            _ann('bone_fusion', 2.0 * B * S * S * 256 * 720, (B * 9 * 80 * 256 + B * S * S * 256) * (4 if self.dtype == F32 else 2) + B * 42 * 2 * 4,
                 'B=%d S=%d factorised bone_proj + 3x3 fusion conv (K=720)' % (B, S))
            _capi.check(L.dir_bone_fusion_forward(st.bone_fusion, _capi.ptr(res['pd_joint_uv_left']),
                                                  _capi.ptr(res['pd_joint_uv_right']), _capi.ptr(scratch),
                                                  _capi.ptr(fused), B, S, st.distance, 256, 0, 1, sp), 'dir_bone_fusion_forward')
            if want_vis:                                        # proj_feat output only (models/dir.py:128,481)
                _ann('proj_feat', 30.0 * B * S * S * 40, B * 1280 * S * S * 4 + B * 42 * 64 * 4, 'B=%d S=%d proj_feat output (fp32 NCHW)' % (B, S))
                _capi.check(L.dir_bone_proj_forward(_capi.ptr(res['pd_joint_uv_left']), _capi.ptr(res['pd_joint_uv_right']),
                                                    _capi.ptr(emb), None, _capi.ptr(vis), None, B, S, st.distance,
                                                    _dt(self.dtype), sp), 'dir_bone_proj_forward')
            st.fusion3(fused, out=img_out, out_coff=img_coff)
        else:
            bone = torch.empty(B, S, S, 2560, device=dev, dtype=self.dtype)
            bbox = torch.empty(B, 40, 4, device=dev, dtype=torch.int32)
            _ann('bone_proj', 30.0 * B * S * S * 40, bone.numel() * bone.element_size() + (B * 1280 * S * S * 4 if want_vis else 0) + B * 42 * 64 * 4,
                 'B=%d S=%d materialised bone map' % (B, S))
            _capi.check(L.dir_bone_proj_forward(_capi.ptr(res['pd_joint_uv_left']), _capi.ptr(res['pd_joint_uv_right']),
                                                _capi.ptr(emb), _capi.ptr(bone), _capi.ptr(vis), _capi.ptr(bbox), B, S,
                                                st.distance, _dt(self.dtype), sp), 'dir_bone_proj_forward')
            st.fusion3(st.fusion0(bone, bbox=bbox if self.sparse_fusion else None), out=img_out, out_coff=img_coff)
        res['joint_feat'] = emb
        res['vis_img_feat'] = vis
        return res

    def _stage_index(self, st):
        """position of the stage's dict in outs_list (0 = the init regression)"""
        return 1 if st is self.stage4 else 2 if st is self.stage3 else 3 + self.stages_x.index(st)

    def upsample_into(self, x, out, coff):
        B, H, W, Cc = x.shape
        _ann('upsample', 0, 5 * x.numel() * x.element_size(), 'B=%d %dx%dx%d -> 2x' % (B, H, W, Cc))
        _capi.check(_capi.lib().dir_upsample2x_bilinear(_capi.ptr(x), _capi.ptr(out), B, H, W, Cc, out.shape[3], coff,
                                                        _dt(self.dtype), _capi.stream_ptr()), 'dir_upsample2x_bilinear')

    factorised_fusion = os.environ.get('DIR_FACTORISED_FUSION', '1') != '0'    # bf16 mode: dir_bone_fusion_forward

    # ------------------------------------------------------------------------------------------ f16x3 calibration
    calibrated = False

    def calibrate(self, img):
        """arith='f16x3' only: one eager forward on `img` during which every convolution records the largest |activation| it reads and
        sets its power-of-two input scale so that this maximum lands in [2^9, 2^10) of the f16 range (include/dir_hip.h: in_scale): 64x
        headroom before values saturate at 65504, full 22-bit operand accuracy down to max / 4096.  Each layer is re-scaled BEFORE it
        runs, so the activations further down are already those of the calibrated network.  Host synchronisations: not capturable; call
        it once per engine on a representative batch (DIR.forward and bench.py do, on the first batch they see).  Without it in_scale is
        1 everywhere: correct for activations inside [2^-3, 65504), saturating beyond."""
        if self.arith is None:
            return
        _TLS.calibrating = True
        try:
            self.forward(img)
            torch.cuda.synchronize(self.device)
        finally:
            _TLS.calibrating = False
        self.calibrated = True

    # ------------------------------------------------------------------------------------------ forward
    _flags = None

    def forward(self, img, want_proj_feat=True, taps=None, reflection_flags=None, want_para=False):
        """img: float32 NCHW [B,3,256,256] on the GPU.  Returns outs_list exactly like DIR.forward (models/dir.py:521-540);
        tensors are engine-owned buffers (valid until the next forward when run under a captured graph).
        want_para: every stage dict also holds pd_mano_para_left / pd_mano_para_right [B,64] (what utils.mano_fit refines; pd_proj_* are views of them).
        reflection_flags: optional int32 tensor [3 (+ extra) stages, 2 hands, B]; an entry is set to 1 where the predicted 6D root rotation
        is a reflection (det < 0) -- where the reference's `assert` fires (rot6d.py:50).  The caller decides when to look (a host
        read); dir_amd.models.dir.DIR.forward does, and raises AssertionError like the reference."""
        _capi.require_cuda(img)
        self._flags = reflection_flags
        _TLS.no_out_split = taps is not None          # the taps are read as fp32 maps
        try:
            return self._forward(img, want_proj_feat, taps, want_para)
        finally:
            self._flags = None
            _TLS.no_out_split = False

    def _forward(self, img, want_proj_feat, taps, want_para=False):
        if img.dtype == torch.uint8:     # decoded BGR frames [B,256,256,3]: the reference's normalisation runs inside the stem staging
            assert img.is_contiguous() and img.shape[1:] == (256, 256, 3)
        else:
            assert img.dtype == F32 and img.is_contiguous() and img.shape[1:] == (3, 256, 256)
        dt, dev = self.dtype, self.device
        B = img.shape[0]
        feats = self.bb(img)
        c1, c2, c3, c4 = feats
        cat4 = torch.empty(B, 16, 16, 2304, device=dev, dtype=dt)
        cat3 = torch.empty(B, 32, 32, 512, device=dev, dtype=dt)
        # everything on the current stream, in one fixed order; the two skip branches depend on the backbone only and come first in their stage
        self.res['skip_layer4'](c3, out=cat4, out_coff=2048)
        init = self.init_regressor(c4)
        # ---- stage 1 @16x16 (models/dir.py:442-456)
        self.upsample_into(c4, cat4, 0)
        enh4_in = torch.empty(B, 16, 16, 512, device=dev, dtype=dt)             # cat(fusion_feat, img_feat)
        self.res['fusion_layer4'](cat4, out=enh4_in, out_coff=0)
        self.res['skip_layer3'](c2, out=cat3, out_coff=256)
        r4 = self.stage(self.stage4, enh4_in, 512, init, enh4_in, 256, False)
        e4 = self.res['enhance_layer4'](enh4_in)
        # ---- stage 2 @32x32 (models/dir.py:459-471)
        self.upsample_into(e4, cat3, 0)
        enh3_in = torch.empty(B, 32, 32, 512, device=dev, dtype=dt)
        self.res['fusion_layer3'](cat3, out=enh3_in, out_coff=0)
        nx = len(self.stages_x)
        r3 = self.stage(self.stage3, enh3_in, 512, r4, enh3_in, 256, want_proj_feat and nx == 0)
        # f4: every further iteration reads the running 32x32 map from channels [0, 256) of its own cat buffer (written there by the
        # previous enhance Residual) and appends its img_feat to channels [256, 512)
        extra, buf, prev = [], enh3_in, r3
        for i in range(nx):
            nxt = torch.empty(B, 32, 32, 512, device=dev, dtype=dt)
            (self.res['enhance_layer3'] if i == 0 else self.res_x[i - 1])(buf, out=nxt, out_coff=0)
            prev = self.stage(self.stages_x[i], nxt, 512, prev, nxt, 256, want_proj_feat and i == nx - 1)
            extra.append(prev)
            buf = nxt
        e3 = (self.res['enhance_layer3'] if nx == 0 else self.res_x[nx - 1])(buf)
        # ---- heads (models/dir.py:474-476)
        feat = self.final_chain(e3)
        sd6 = self.heads_chain(feat)                                             # NHWC fp32 [B,32,32,6] = seg | dense
        seg, dense = sd6[..., :3], sd6[..., 3:]
        if taps is not None:
            taps.update(c1=c1, c2=c2, c3=c3, c4=c4, fusion4=enh4_in[..., :256], proj4=enh4_in[..., 256:], enh4=e4,
                        fusion3=enh3_in[..., :256], proj3=enh3_in[..., 256:], enh3=e3, final=feat,
                        skip4=cat4[..., 2048:])
        outs = []
        for o in [init, r4, r3] + extra:
            outs.append({k: o[k] for k in ('pd_joint_uv_left', 'pd_joint_uv_right', 'pd_mesh_xyz_left',
                                           'pd_mesh_xyz_right', 'pd_joint_xyz_left', 'pd_joint_xyz_right',
                                           'pd_proj_left', 'pd_proj_right', 'pd_offset', 'pd_rel_joint') + (('pd_mano_para_left', 'pd_mano_para_right') if want_para else ())})
        outs.append({'dense': dense.permute(0, 3, 1, 2), 'seg': seg.permute(0, 3, 1, 2),
                     'proj_feat': (extra[-1] if extra else r3)['vis_img_feat']})
        return outs
