"""Weight streams of the kernels that read their MFMA A operand in consumption order (include/dir_hip.h): pure index gathers, no library call."""
import torch


def pack_as_weights(w_ohwi, A):
    """dir_conv2d_as_forward's weight stream (include/dir_hip.h) from W [Cout][kh][kw][Cin] (16-bit): [Cout / (128 A)][4 waves][kh kw Cin / 64 steps]
    [4 k-steps][A][64 lanes][8], step = (64-channel slab) * (kh kw) + tap -- every wave's MFMA A fragments in the order it consumes them, with the
    k-slot assignment of conv.hip's MFMAs (lanes 0-31: channels 8 ks .. + 8 of the slab, lanes 32-63: 32 + 8 ks .. + 8)."""
    N, kh, kw, Cin = w_ohwi.shape
    assert N % (128 * A) == 0 and Cin % 64 == 0
    nt = kh * kw
    dev = w_ohwi.device
    w = w_ohwi.reshape(N, nt * Cin)
    lane = torch.arange(64, device=dev)
    l32, h = lane & 31, lane >> 5
    e = torch.arange(8, device=dev)
    g, wv, st, ks, cb = torch.meshgrid(torch.arange(N // (128 * A), device=dev), torch.arange(4, device=dev), torch.arange(nt * Cin // 64, device=dev),
                                       torch.arange(4, device=dev), torch.arange(A, device=dev), indexing='ij')
    row = (g * (128 * A) + (wv * A + cb) * 32)[..., None] + l32                       # [G,4,steps,4,A,64]
    slab, tap = st // nt, st % nt
    k0 = (tap * Cin + 64 * slab + 8 * ks)[..., None] + 32 * h
    return w[row[..., None], k0[..., None] + e].contiguous()


def pack_stream_weights(w_nk, dtype=torch.bfloat16):
    """dir_conv1x1_stream_forward's weight stream (include/dir_hip.h) from W [Cout, K] (K = Cin, or Cin + Cin2 for two sources):
    `dtype` [Cout/NWG][4 waves][K/64][4 k-steps][NCB][64 lanes][8] -- pack_as_weights' layout for a single tap, NCB = 2 where Cout allows it."""
    N, K = w_nk.shape
    assert N % 128 == 0 and K % 64 == 0
    return pack_as_weights(w_nk.detach().to(dtype).reshape(N, 1, 1, K), 2 if N % 256 == 0 else 1)


def pack_l3_stream(w2_ohwi, w3, w1n=None, dtype=torch.bfloat16):
    """dir_bottleneck_block_forward's weight stream (include/dir_hip.h) from conv2.weight [256][3][3][256] (NHWC-ordered, as ConvOp keeps it),
    conv3.weight [1024, 256] and the next conv1.weight [256, 1024] (or None): per wave its 144 conv2 fragments (pack_as_weights with one block
    per wave), then per 512-channel half its conv3 and conv1 fragments -- pack_tail_stream's where the next conv1 is fused, a convolution's
    k-slots for conv3 where it is not (the launch replaced is then a convolution).  [8 waves][144 + 2 (32 + NCF)][64 lanes][8]."""
    w2 = w2_ohwi.detach().to(dtype)
    w3 = w3.detach().reshape(w3.shape[0], -1).to(dtype)
    assert tuple(w2.shape) == (256, 3, 3, 256) and tuple(w3.shape) == (1024, 256)
    a = pack_as_weights(w2, 1).reshape(8, 144, 64, 8)                              # [2 slices][4 waves] = channel block 32 w
    if w1n is not None:
        u = pack_tail_stream(w3, w1n, 8, dtype=dtype).to(w2.device).reshape(2, 8, 64, 64, 8)
    else:                                                                          # [32 channel blocks = (half, wave, cb)][4 slabs][4 k-steps]
        u = pack_as_weights(w3.reshape(1024, 1, 1, 256), 1).reshape(2, 8, 32, 64, 8)
    return torch.cat([a, u[0], u[1]], 1).contiguous()


def pack_tail_stream(w3, w1n, waves=8, dtype=torch.bfloat16):
    """dir_bottleneck_tail_forward's weight stream (include/dir_hip.h): conv3.weight [4P, P] and the next conv1.weight [N2, 4P]
    as bf16 MFMA A-operand fragments in the order the kernel's waves consume them, [4P/512][waves][NBF + NCF][64 lanes][8]
    (waves = 8: 64-pixel tiles, one workgroup per CU; waves = 4: the thin variant, 32-pixel tiles, two workgroups per CU)."""
    out_dev = w3.device
    w3 = w3.detach().float().reshape(w3.shape[0], -1).cpu()        # packed on the host: hundreds of small gathers, once per engine
    w1n = w1n.detach().float().reshape(w1n.shape[0], -1).cpu()
    C4, P = w3.shape
    N2 = w1n.shape[0]
    assert w1n.shape[1] == C4 and C4 == 4 * P and C4 % 512 == 0 and N2 in (128, 256)
    dev = w3.device
    lane = torch.arange(64, device=dev)
    l32, h, l16, g16 = lane & 31, lane >> 5, lane & 15, lane >> 4
    e = torch.arange(8, device=dev)
    KBS = P // 16
    out = []
    if waves == 4:
        ncc = N2 // 128
        for hf in range(C4 // 512):
            for w in range(4):
                for cb in range(4):
                    for ks in range(KBS):
                        out.append(w3[(hf * 512 + 128 * w + 32 * cb + l32)[:, None], (16 * ks + 8 * h)[:, None] + e])
                for ks in range(32):
                    for cc in range(ncc):
                        out.append(w1n[((N2 // 4) * w + 32 * cc + l32)[:, None], (hf * 512 + 16 * ks + 8 * h)[:, None] + e])
        return torch.stack(out).to(dtype).contiguous().to(out_dev)
    for hf in range(C4 // 512):
        for w in range(8):
            for cb in range(2):
                for ks in range(KBS):
                    ch = hf * 512 + 64 * w + 32 * cb + l32
                    k0 = 16 * ks + 8 * h
                    out.append(w3[ch[:, None], k0[:, None] + e])
            if N2 == 128:
                for fc in range(16):
                    out.append(w1n[(16 * w + l16)[:, None], (hf * 512 + 32 * fc + 8 * g16)[:, None] + e])
            else:
                for fc in range(32):
                    out.append(w1n[(32 * w + l32)[:, None], (hf * 512 + 16 * fc + 8 * h)[:, None] + e])
    return torch.stack(out).to(dtype).contiguous().to(out_dev)
