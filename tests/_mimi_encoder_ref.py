"""CPU checker of the Mimi encoder -- PARITY UNPINNED: inferred architecture, no reference fixture.

The reference has no native encoder (mimi.go:14,791-794: ErrMimiEncoderNotImplemented); the chain exists only inside the exported ONNX graph.
This is an independent restatement, in float64 torch on the CPU, of the chain as DESIGN.md section 7 infers it from the decoder:

    head    causal conv 1 -> f, stride 1                       encoder.model.0.conv
    res j   x + c1(elu(c3(elu(x))))                            encoder.model.{1,4,7}.block.{1,3}.conv
    down j  elu, then causal conv with stride = kernel / 2     encoder.model.{3,6,9}.conv
    tail    elu, then causal conv 8f -> mimi_dim, stride 1     encoder.model.11.conv
    transformer: the decoder transformer's layer (LayerNorm, interleaved-pair RoPE from position 0, causal window of 250 keys, layer scale,
                 GELU feed-forward)                            encoder_transformer.transformer.layers.N
    downsample  causal conv, stride = kernel / 2, no bias      downsample.conv.conv

Every conv is causal with zero history: a stride-s, kernel-k conv sees k - s zero samples before t = 0, so output t covers input
[t s - (k - s), t s + s).  The clip is zero-padded at its end to a whole number of frames (hop = product of the strides).  The output is the raw
[frames, mimi_dim] latent.  Written from that description, not from the HIP code.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

P = "mimi."
EM = P + "encoder.model."
STAGES = ("head", "res1", "down1", "res2", "down2", "res3", "down3", "tail", "transformer", "latent")


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def conv1d(x, w, b, stride=1, lpad=0):
    """x [Cin, L], w [Cout, Cin, k] -> [Cout, floor((L + lpad - k) / stride) + 1]"""
    x = F.pad(_t(x), (lpad, 0))
    return F.conv1d(x[None], _t(w), None if b is None else _t(b), stride=stride)[0]


def causal_conv(x, w, b, stride=1):
    """Causal conv with zero history: k - stride zeros in front."""
    return conv1d(x, w, b, stride, w.shape[-1] - stride)


def elu(x):
    return F.elu(x)


def frames_of(n_samples, hop=1920):
    return -(-n_samples // hop)


class EncoderRef:
    def __init__(self, tensors, heads=8, context=250):
        self.t = {k: v for k, v in tensors.items() if k.startswith(P)}
        self.heads, self.context = heads, context
        self.dim = self.t[EM + "11.conv.weight"].shape[0]
        self.strides = [self.t[f"{EM}{i}.conv.weight"].shape[-1] // 2 for i in (3, 6, 9)]
        self.ds = self.t[P + "downsample.conv.conv.weight"].shape[-1] // 2
        self.hop = self.strides[0] * self.strides[1] * self.strides[2] * self.ds
        self.layers = 0
        while f"{P}encoder_transformer.transformer.layers.{self.layers}.norm1.weight" in self.t:
            self.layers += 1

    def w(self, name):
        return self.t[name + ".weight"], self.t.get(name + ".bias")

    # ---------------------------------------------------------------- stages
    def head(self, pcm):
        n = pcm.size
        x = np.zeros(frames_of(n, self.hop) * self.hop)
        x[:n] = pcm
        return causal_conv(x[None], *self.w(EM + "0.conv"))

    def resblock(self, x, idx):
        h = causal_conv(elu(x), *self.w(f"{EM}{idx}.block.1.conv"))
        return x + causal_conv(elu(h), *self.w(f"{EM}{idx}.block.3.conv"))

    def down(self, x, idx, stride):
        return causal_conv(elu(x), *self.w(f"{EM}{idx}.conv"), stride=stride)

    def tail(self, x):
        return causal_conv(elu(x), *self.w(EM + "11.conv"))

    def layer(self, x, i):
        """One transformer layer on rows x [T, D]."""
        p = f"{P}encoder_transformer.transformer.layers.{i}"
        return transformer_layer(x, {k[len(p) + 1:]: v for k, v in self.t.items() if k.startswith(p + ".")}, self.heads, self.context)

    def transformer(self, x_rows):
        for i in range(self.layers):
            x_rows = self.layer(x_rows, i)
        return x_rows

    def downsample(self, x_rows):
        return causal_conv(x_rows.T, self.t[P + "downsample.conv.conv.weight"], None, stride=self.ds).T

    # ---------------------------------------------------------------- whole chain
    def stages(self, pcm):
        """The ten observation points, channels-last numpy float64: the residual stages after the ELU their readers apply."""
        out = {}
        x = self.head(np.asarray(pcm, np.float64))
        out["head"] = x
        for j, (ri, di) in enumerate(((1, 3), (4, 6), (7, 9))):
            r = self.resblock(x, ri)
            out[f"res{j + 1}"] = elu(r)
            x = self.down(r, di, self.strides[j])
            out[f"down{j + 1}"] = x
        x = self.tail(x).T
        out["tail"] = x.T
        x = self.transformer(x)
        out["transformer"] = x.T
        out["latent"] = self.downsample(x).T
        return {k: v.T.numpy() for k, v in out.items()}

    def encode(self, pcm):
        x = self.head(np.asarray(pcm, np.float64))
        for j, (ri, di) in enumerate(((1, 3), (4, 6), (7, 9))):
            x = self.down(self.resblock(x, ri), di, self.strides[j])
        return self.downsample(self.transformer(self.tail(x).T)).numpy()


def rope(x, heads):
    """Interleaved-pair rotation of rows x [T, heads * hd] at positions 0 .. T-1 (max period 10000)."""
    T, D = x.shape
    hd = D // heads
    half = hd // 2
    inv = 1.0 / (10000.0 ** (torch.arange(half, dtype=torch.float64) / half))
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None, :]
    c, s = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    xr = x.reshape(T, heads, half, 2)
    a, b = xr[..., 0], xr[..., 1]
    return torch.stack((a * c - b * s, a * s + b * c), dim=-1).reshape(T, D)


def transformer_layer(x, w, heads, context):
    """The Mimi transformer layer on rows x [T, D]; w: the layer's tensors without their prefix."""
    x = _t(x)
    T, D = x.shape
    hd = D // heads
    g = lambda n: _t(w[n])
    h = F.layer_norm(x, (D,), g("norm1.weight"), g("norm1.bias"), 1e-5)
    qkv = h @ g("self_attn.in_proj.weight").T
    q, k, v = rope(qkv[:, :D], heads), rope(qkv[:, D:2 * D], heads), qkv[:, 2 * D:]
    q, k, v = (a.reshape(T, heads, hd).transpose(0, 1) for a in (q, k, v))
    o = torch.empty(heads, T, hd, dtype=torch.float64)
    for r0 in range(0, T, 512):   # query rows in blocks: query p sees keys j with p - context < j <= p
        r1 = min(T, r0 + 512)
        k0 = max(0, r0 - context + 1)
        pq, pk = torch.arange(r0, r1), torch.arange(k0, r1)
        allowed = (pk[None, :] <= pq[:, None]) & (pk[None, :] > pq[:, None] - context)
        sc = (q[:, r0:r1] @ k[:, k0:r1].transpose(1, 2)) / math.sqrt(hd)
        sc = sc.masked_fill(~allowed[None], float("-inf"))
        o[:, r0:r1] = torch.softmax(sc, dim=-1) @ v[:, k0:r1]
    o = o.transpose(0, 1).reshape(T, D) @ g("self_attn.out_proj.weight").T
    x = x + (g("layer_scale_1.scale") * o if "layer_scale_1.scale" in w else o)
    h = F.layer_norm(x, (D,), g("norm2.weight"), g("norm2.bias"), 1e-5)
    y = F.gelu(h @ g("linear1.weight").T) @ g("linear2.weight").T
    return x + (g("layer_scale_2.scale") * y if "layer_scale_2.scale" in w else y)
