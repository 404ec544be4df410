"""Plain f64 host references of the detector / segmenter kernels (csrc/sam_ops.hip, the deformable-attention part of
csrc/detect_ops.hip), written from the formulas and not from the kernels.  tests/test_detect_ref_cpu.py pins each of them to the
framework on the CPU; the -m gpu tests compare the HIP kernels with them."""
import torch
import torch.nn.functional as F


def window_attention_f64(qkv, bias, mask, heads, scale):
    """softmax(scale * q k^T + bias[h] + mask[w mod W]) v per (window, head), head width 32.  qkv [windows, tokens, heads * 96] with
    q | k | v per head, bias [heads, tokens, tokens] (query, key), mask [W, tokens, tokens] (query, key) or None.  Returns
    (out [windows, tokens, heads * 32], scores [windows, heads, tokens, tokens]) in f64."""
    nw, n, _ = qkv.shape
    q, k, v = qkv.double().view(nw, n, heads, 3, 32).permute(3, 0, 2, 1, 4)          # each [windows, heads, tokens, 32]
    s = scale * (q @ k.transpose(2, 3)) + bias.double()[None]
    if mask is not None:
        s = s + mask.double()[torch.arange(nw) % mask.shape[0]][:, None]
    p = torch.softmax(s, dim=-1)
    return (p @ v).transpose(1, 2).reshape(nw, n, heads * 32), s


def layernorm_windows_f64(x, gamma, beta, eps, window, shift, pad_zero):
    """LayerNorm over the channels of x [B, H, W, C]; window > 0: then pad to multiples of the window at the bottom / right (with 0
    when pad_zero, else with beta = LayerNorm(0)), roll by -shift along both axes, partition -> [B * nWy * nWx, window^2, C]."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    if window <= 0:
        return y
    B, H, W, C = y.shape
    ph, pw = (window - H % window) % window, (window - W % window) % window
    if pad_zero:
        y = F.pad(y, (0, 0, 0, pw, 0, ph))
    else:
        full = beta.double().expand(B, H + ph, W + pw, C).clone()
        full[:, :H, :W] = y
        y = full
    if shift:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    hp, wp = H + ph, W + pw
    return y.view(B, hp // window, window, wp // window, window, C).transpose(2, 3).reshape(-1, window * window, C)


def window_reverse_f64(x, windows, window, shift):
    """x [B, H, W, C] + (windows [B * nWy * nWx, window^2, C] merged, rolled back by +shift, cropped to H x W).  The result keeps
    the dtype of its operands promoted to f64; on f32 inputs `.float()` of it is the one f32 addition."""
    B, H, W, C = x.shape
    hp, wp = (H + window - 1) // window * window, (W + window - 1) // window * window
    a = windows.view(B, hp // window, wp // window, window, window, C).transpose(2, 3).reshape(B, hp, wp, C)
    if shift:
        a = torch.roll(a, shifts=(shift, shift), dims=(1, 2))
    return x.double() + a[:, :H, :W].double()


def dwconv3x3_nhwc_f64(x, w, bias):
    """Depthwise 3x3, stride 1, zero padding 1, on x [B, H, W, C]; w [C, 1, 3, 3]; bias [C] or None.  Nine shifted products."""
    B, H, W, C = x.shape
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    out = torch.zeros(B, H, W, C, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            out += xp[:, dy:dy + H, dx:dx + W] * w.double()[:, 0, dy, dx]
    return out if bias is None else out + bias.double()


def ms_deform_attn_f64(value, shapes, level_start, loc, w):
    """Multi-scale deformable attention sampling: out[b, q, h * D + d] = sum_{l, p} w[b, q, h, l, p] * bilinear(value_l[b, :, h, d],
    loc[b, q, h, l, p]) with grid_sample's align_corners = False convention (pixel centres at (i + 0.5) / size) and zero padding,
    as an explicit four-tap gather.  value [B, S, heads, D], loc [B, Q, heads, L, P, 2] (x, y), w [B, Q, heads, L, P].
    Returns (out [B, Q, heads * D], sum of the absolute values of the terms, same shape), f64."""
    B, S, heads, D = value.shape
    _, Q, _, L, P, _ = loc.shape
    value, loc, w = value.double(), loc.double(), w.double()
    out = torch.zeros(B, Q, heads, D, dtype=torch.float64)
    mag = torch.zeros_like(out)
    bi = torch.arange(B).view(B, 1, 1, 1)
    hi = torch.arange(heads).view(1, 1, heads, 1)
    for l, (Hl, Wl) in enumerate(shapes):
        s0 = int(level_start[l])
        x = loc[:, :, :, l, :, 0] * Wl - 0.5                                       # [B, Q, heads, P]
        y = loc[:, :, :, l, :, 1] * Hl - 0.5
        x0, y0 = torch.floor(x), torch.floor(y)
        tx, ty = x - x0, y - y0
        for dy, dx, k in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)), (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
            xi, yi = x0.long() + dx, y0.long() + dy
            inside = (xi >= 0) & (xi < Wl) & (yi >= 0) & (yi < Hl)
            idx = s0 + yi.clamp(0, Hl - 1) * Wl + xi.clamp(0, Wl - 1)
            tap = value[bi, idx, hi]                                                # [B, Q, heads, P, D]
            term = tap * (k * inside * w[:, :, :, l])[..., None]
            out += term.sum(3)
            mag += term.abs().sum(3)
    return out.reshape(B, Q, heads * D), mag.reshape(B, Q, heads * D)


def deform_locations_f64(offsets_logits, ref, shapes, heads, L, P):
    """The softmax and the sampling-location arithmetic in front of the sampling, f64: offsets_logits [B, Q, heads * L * P * 3] =
    offsets [h][l][p][2] then logits [h][l][p]; ref [B, Q, L, 2 | 4].  Returns (loc [B, Q, heads, L, P, 2], w [B, Q, heads, L, P])."""
    B, Q, _ = offsets_logits.shape
    ol = offsets_logits.double()
    off = ol[..., :heads * L * P * 2].view(B, Q, heads, L, P, 2)
    w = torch.softmax(ol[..., heads * L * P * 2:].view(B, Q, heads, L * P), -1).view(B, Q, heads, L, P)
    r = ref.double()[:, :, None, :, None, :]
    if ref.shape[-1] == 2:
        norm = torch.tensor([[float(wl), float(hl)] for hl, wl in shapes], dtype=torch.float64)
        loc = r + off / norm[None, None, None, :, None, :]
    else:
        loc = r[..., :2] + off / P * r[..., 2:] * 0.5
    return loc, w


def ms_deform_attn_fused_f64(value, shapes, level_start, offsets_logits, ref, L, P):
    """deform_locations_f64 followed by ms_deform_attn_f64.  Returns (out, sum of absolute values)."""
    loc, w = deform_locations_f64(offsets_logits, ref, shapes, value.shape[2], L, P)
    return ms_deform_attn_f64(value, shapes, level_start, loc, w)


# ------------------------------------------------------------------------------------------------ shared case builders
def level_starts(shapes):
    starts, s = [], 0
    for h, w in shapes:
        starts.append(s)
        s += h * w
    return torch.tensor(starts), s


def exact_coordinates(size):
    """The sampling coordinates where a bilinear gather goes wrong: 0, 1, the first / last pixel centre, the first / last interior
    pixel edge, half a pixel outside on either side.  (For a level of size 1 several of them coincide.)"""
    s = float(size)
    return [0.0, 1.0, 0.5 / s, 1 - 0.5 / s, 1 / s, (s - 1) / s, -0.5 / s, 1 + 0.5 / s]


def swin_like_mask(tokens, positions, gen):
    """A shifted-window style additive mask [positions, tokens, tokens] (query, key) of 0 / -100 from random region labels; window
    position 0 additionally hides keys 0-31 from queries >= 32 (the first key tile of an online softmax then carries almost no
    weight); a few ONE-SIDED -100 entries make it non-symmetric; every query keeps its own key (diagonal 0)."""
    labels = torch.randint(0, 3, (positions, tokens), generator=gen)
    mask = (labels[:, :, None] != labels[:, None, :]).double() * -100.0
    if tokens > 32:
        mask[0, 32:, :32] = -100.0
    for w in range(positions):
        for _ in range(max(1, tokens // 8)):
            i, j = (int(t) for t in torch.randint(0, tokens, (2,), generator=gen))
            if i != j:
                mask[w, i, j] = -100.0
                mask[w, j, i] = 0.0
    idx = torch.arange(tokens)
    mask[:, idx, idx] = 0.0
    return mask.float()
