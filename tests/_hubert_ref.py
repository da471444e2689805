"""Plain torch mirror of HuBERT-base as gsv/feature_extractor/cnhubert.py's docstring describes it, on a state dict with
transformers.HubertModel's keys (gsv.synthetic.make_hubert_state_dict): 7 bias-free convs (kernels 10,3,3,3,3,2,2, strides
5,2,2,2,2,2,2), GroupNorm(512, 512) after the first, GELU after each; LayerNorm + Linear 512 -> 768; the weight-normed grouped
positional conv (k = 128, 16 groups, padding 64, last frame dropped) + GELU, added; LayerNorm; 12 post-LN layers.  fp32 or fp64.
The reference of the packed-pass tests; tests/test_hubert_pack.py pins it against tests/golden/hubert_base.npz."""
import torch
import torch.nn.functional as F

KERNELS = (10, 3, 3, 3, 3, 2, 2)
STRIDES = (5, 2, 2, 2, 2, 2, 2)


def _sd(sd, dtype):
    return {(k[7:] if k.startswith("hubert.") else k): v.detach().to(dtype) for k, v in sd.items() if torch.is_tensor(v)}


@torch.no_grad()
def conv_stack(sd, wav, dtype=torch.float64, gn_segments=None, eps=1e-5):
    """wav [n] -> [T, 512] after the 7 convs.  gn_segments: (first row, rows) ranges of conv 0's output; GroupNorm's statistics
    run over each range on its own and rows outside every range become 0.  None: one range over all rows."""
    sd = _sd(sd, dtype)
    h = F.conv1d(wav.to(dtype).view(1, 1, -1), sd["feature_extractor.conv_layers.0.conv.weight"], stride=STRIDES[0])[0]   # [512, T0]
    gw, gb = sd["feature_extractor.conv_layers.0.layer_norm.weight"], sd["feature_extractor.conv_layers.0.layer_norm.bias"]
    out = torch.zeros_like(h)
    for a, n in (gn_segments if gn_segments is not None else [(0, h.shape[1])]):
        seg = h[:, a:a + n]
        mean, var = seg.mean(1, keepdim=True), seg.var(1, unbiased=False, keepdim=True)
        out[:, a:a + n] = (seg - mean) / torch.sqrt(var + eps) * gw[:, None] + gb[:, None]
    h = F.gelu(out)
    for i in range(1, 7):
        h = F.gelu(F.conv1d(h[None], sd[f"feature_extractor.conv_layers.{i}.conv.weight"], stride=STRIDES[i])[0])
    return h.t().contiguous()


@torch.no_grad()
def feature_projection(sd, h, dtype=torch.float32, eps=1e-5):
    """conv stack output [T, 512] -> LayerNorm -> Linear: [T, 768] (row-wise)"""
    sd = _sd(sd, dtype)
    h = F.layer_norm(h, (h.shape[1],), sd["feature_projection.layer_norm.weight"], sd["feature_projection.layer_norm.bias"], eps)
    return F.linear(h, sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"])


@torch.no_grad()
def positional(sd, h, dtype=torch.float32, eps=1e-5):
    """projected features [T, 768] -> (pos = GELU(grouped conv, k = 128, padding 64, last frame dropped), LayerNorm(h + pos))"""
    sd = _sd(sd, dtype)
    T, hid = h.shape
    pre = "encoder.pos_conv_embed.conv."
    if pre + "parametrizations.weight.original0" in sd:
        g, v = sd[pre + "parametrizations.weight.original0"], sd[pre + "parametrizations.weight.original1"]
        pw = v * (g / v.norm(dim=(0, 1), keepdim=True))
    elif pre + "weight_g" in sd:
        g, v = sd[pre + "weight_g"], sd[pre + "weight_v"]
        pw = v * (g / v.norm(dim=(0, 1), keepdim=True))
    else:
        pw = sd[pre + "weight"]
    k = pw.shape[2]
    pos = F.conv1d(h.t()[None], pw, sd[pre + "bias"], padding=k // 2, groups=hid // pw.shape[1])[0][:, :T]
    pos = F.gelu(pos).t()
    return pos, F.layer_norm(h + pos, (hid,), sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"], eps)


@torch.no_grad()
def hubert(sd, wav, dtype=torch.float32, layers=12, heads=12, eps=1e-5):
    """wav [n] -> dict(last_hidden_state, pos, enc_in), each [T, 768]"""
    h = feature_projection(sd, conv_stack(sd, wav, dtype), dtype)
    pos, x = positional(sd, h, dtype)
    sd = _sd(sd, dtype)
    T, hid = x.shape
    enc_in = x
    hd = hid // heads
    for i in range(layers):
        p = f"encoder.layers.{i}."
        q, kk, v = (F.linear(x, sd[p + f"attention.{n}.weight"], sd[p + f"attention.{n}.bias"]).view(T, heads, hd).transpose(0, 1)
                    for n in ("q_proj", "k_proj", "v_proj"))
        a = torch.softmax(q @ kk.transpose(1, 2) * hd ** -0.5, -1) @ v
        a = a.transpose(0, 1).reshape(T, hid)
        o = F.linear(a, sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"]) + x
        x = F.layer_norm(o, (hid,), sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], eps)
        f = F.gelu(F.linear(x, sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"]))
        f = F.linear(f, sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"]) + x
        x = F.layer_norm(f, (hid,), sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], eps)
    return {"last_hidden_state": x, "pos": pos, "enc_in": enc_in}


# the eight lengths of the packed-pass tests: one-frame audios (400, 719), the first two-frame one (720), the golden's (20800),
# slots that are whole hops (41600, 8000, 640) and one that is not (48079)
LENGTHS = (400, 719, 720, 20800, 41600, 8000, 48079, 640)
GOLDEN_INDEX, GOLDEN_SEED = 3, 7


def waveforms():
    """the eight test audios: make_waveform(20800, 7) is the golden's, the others have seeds of their own"""
    from gsv import synthetic as S
    return [S.make_waveform(n, GOLDEN_SEED if i == GOLDEN_INDEX else 20 + i) for i, n in enumerate(LENGTHS)]
