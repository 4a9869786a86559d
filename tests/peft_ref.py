"""The image encoder of oracle/sam_ref.py with a PEFT method of the reference (micro_sam/models/peft_sam.py) applied as a SEPARATE BRANCH,
in the oracle's arithmetic: ``image_encoder_peft`` restates the oracle's block loop, takes an UN-MERGED state dict with the reference's
names and evaluates

* ``"fact"``         ``qkv_proj(x)``, plus ``FacTv(q_FacTs(FacTu(x)))`` on the q columns and the same with ``v_FacTs`` on the v columns;
* ``"ssf"``          every wrapped linear layer and LayerNorm, then ``* scale + shift``;
* ``"adaptformer"``  ``x + [y + mlp_proj(y) + alpha (relu(y Wd^T + bd) Wu^T + bu)]`` with ``y = norm2(x)`` - the adapter's own residual is
                     its input, the normed stream.  In the "bf16" policy the branch rounds where csrc/adapter.hip does: y (the 16-bit
                     LayerNorm output the kernel reads, also as the added term), the two weights, and the hidden once (the MLP hidden's site).

Blocks without keys of the method are plain.  With no PEFT keys at all the loop IS the oracle's (tests/test_gpu_peft_methods.py checks
``torch.equal`` taps), which is what lets the restatement stand in for it.  ``merged_state_dict`` gives the plain state dict a FacT / SSF
model equals (the merge identities of DESIGN.md), formed in fp32."""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import sam_ref as S
from oracle.sam_ref import Prec, _attention_relpos, _window_partition, _window_unpartition

Tensor = torch.Tensor


class _BranchPrec(Prec):
    """The oracle's rounding policy whose four large projections take a per-site hook ``(x, y) -> y'`` (the PEFT branch of that site)."""

    def __init__(self, precision: str):
        super().__init__(precision)
        self.hooks = {}

    def linear_q(self, x, w, b=None, src="fp32", esite=None):
        y = super().linear_q(x, w, b, src=src, esite=esite)
        hook = self.hooks.get(esite)
        return y if hook is None else hook(x, y)


def _ssf(sd, pre):
    scale, shift = sd[pre + "scale"], sd[pre + "shift"]
    return lambda x, y: y * scale + shift


def image_encoder_peft(sd: Dict[str, Tensor], x: Tensor, method: Optional[str] = None, stop_after_block: Optional[int] = None,
                       model_type: str = "vit_b", precision: str = "fp32"):
    """-> (embedding [B, 256, 64, 64] or None when stopped, [residual stream after block 0, 1, ...])."""
    assert method in (None, "fact", "ssf", "adaptformer"), method
    cfg = S.VIT_CONFIGS[model_type[:5]]
    p = _BranchPrec(precision)
    pre = "image_encoder."
    D, heads = cfg["embed_dim"], cfg["num_heads"]
    w = sd[pre + "patch_embed.proj.weight"]
    p.block = -1
    x = F.conv2d(p.re(x, "patch"), p.re(w, "patch"), None, stride=S.PATCH) + sd[pre + "patch_embed.proj.bias"].view(1, -1, 1, 1)
    x = x.permute(0, 2, 3, 1)
    x = x + sd[pre + "pos_embed"]
    taps = []
    for i in range(cfg["depth"]):
        bp = f"{pre}blocks.{i}."
        p.block = i
        p.hooks = {}
        fact = bp + "attn.qkv.FacTu.weight" in sd
        ssf = bp + "norm1.scale" in sd
        adapt = bp + "mlp.down_proj.weight" in sd
        assert (fact, ssf, adapt) == (fact and method == "fact", ssf and method == "ssf", adapt and method == "adaptformer"), (i, method)
        blk = {k[len(bp):]: v for k, v in sd.items() if k.startswith(bp)}       # the block's keys under the plain names
        if fact:
            a = "attn.qkv."
            blk[a + "weight"], blk[a + "bias"] = blk[a + "qkv_proj.weight"], blk[a + "qkv_proj.bias"]

            def fact_branch(xin, y, a=a, blk=blk):
                low = p.linear(xin, blk[a + "FacTu.weight"], esite="qkv")
                new_q = p.linear(p.linear(low, blk[a + "q_FacTs.weight"], esite="qkv"), blk[a + "FacTv.weight"], esite="qkv")
                new_v = p.linear(p.linear(low, blk[a + "v_FacTs.weight"], esite="qkv"), blk[a + "FacTv.weight"], esite="qkv")
                return y + torch.cat([new_q, torch.zeros_like(new_q), new_v], dim=-1)
            p.hooks["qkv"] = fact_branch
        if ssf:
            for name, site in (("attn.qkv.", "qkv"), ("attn.proj.", "proj"), ("mlp.lin1.", "lin1"), ("mlp.lin2.", "lin2")):
                blk[name + "weight"], blk[name + "bias"] = blk[name + "layer.weight"], blk[name + "layer.bias"]
                p.hooks[site] = _ssf(blk, name)
            for name in ("norm1.", "norm2."):
                blk[name + "weight"], blk[name + "bias"] = blk[name + "layer.weight"], blk[name + "layer.bias"]
        if adapt:
            for j in ("1", "2"):
                blk[f"mlp.lin{j}.weight"], blk[f"mlp.lin{j}.bias"] = blk[f"mlp.mlp_proj.lin{j}.weight"], blk[f"mlp.mlp_proj.lin{j}.bias"]

        shortcut = x
        y = F.layer_norm(x, (D,), blk["norm1.weight"], blk["norm1.bias"], eps=1e-6)
        if ssf:
            y = y * blk["norm1.scale"] + blk["norm1.shift"]
        if i in cfg["global_attn_indexes"]:
            y = _attention_relpos(blk, "attn.", y, heads, p)
        else:
            H, W = y.shape[1:3]
            y, pad_hw = _window_partition(y, S.WINDOW)
            y = _attention_relpos(blk, "attn.", y, heads, p)
            y = _window_unpartition(y, S.WINDOW, pad_hw, (H, W))
        x = shortcut + y
        y = F.layer_norm(x, (D,), blk["norm2.weight"], blk["norm2.bias"], eps=1e-6)
        if ssf:
            y = y * blk["norm2.scale"] + blk["norm2.shift"]
        n2 = y
        y = p.linear_q(y, blk["mlp.lin1.weight"], blk["mlp.lin1.bias"], src="fp32", esite="lin1")
        y = F.gelu(y)
        y = p.linear_q(y, blk["mlp.lin2.weight"], blk["mlp.lin2.bias"], src="bf16", esite="lin2")
        x = x + y
        if adapt:
            y16 = p.re(n2, "lin1.x")                                             # the LayerNorm output as the kernel reads it
            h = torch.relu(F.linear(y16, p.re(blk["mlp.down_proj.weight"], "lin1.w")) + blk["mlp.down_proj.bias"])
            up = F.linear(p.re(h, "lin2.x"), p.re(blk["mlp.up_proj.weight"], "lin2.w")) + blk["mlp.up_proj.bias"]
            alpha = blk["mlp.alpha"] if "mlp.alpha" in blk else 1.0
            x = x + (y16 + alpha * up)
        taps.append(x.clone())
        if stop_after_block is not None and i == stop_after_block:
            return None, taps
    x = x.permute(0, 3, 1, 2)
    p.block = cfg["depth"]
    x = F.conv2d(p.re(x, "neck"), p.re(sd[pre + "neck.0.weight"], "neck"))
    x = S.layer_norm_2d(x, sd[pre + "neck.1.weight"], sd[pre + "neck.1.bias"])
    x = F.conv2d(p.re(x, "neck"), p.re(sd[pre + "neck.2.weight"], "neck"), padding=1)
    x = S.layer_norm_2d(x, sd[pre + "neck.3.weight"], sd[pre + "neck.3.bias"])
    return x, taps


def merged_state_dict(sd: Dict[str, Tensor], method: str, device="cpu") -> Dict[str, Tensor]:
    """The plain state dict a FacT / SSF state dict equals, formed in fp32 on ``device`` (returned on the CPU)."""
    assert method in ("fact", "ssf"), method
    out = {}
    f = lambda t: t.to(device=device, dtype=torch.float32)
    for k, v in sd.items():
        if method == "fact" and ".attn.qkv." in k and k.startswith("image_encoder.blocks."):
            a = k[:k.index(".attn.qkv.") + len(".attn.qkv.")]
            if a + "FacTu.weight" not in sd:
                out[k] = v
            elif k == a + "qkv_proj.weight":
                w = f(v).clone()
                Dm = w.shape[1]
                u, vv = f(sd[a + "FacTu.weight"]), f(sd[a + "FacTv.weight"])
                w[:Dm] += vv @ f(sd[a + "q_FacTs.weight"]) @ u
                w[2 * Dm:] += vv @ f(sd[a + "v_FacTs.weight"]) @ u
                out[a + "weight"] = w.cpu()
            elif k == a + "qkv_proj.bias":
                out[a + "bias"] = v
        elif method == "ssf" and k.endswith(".layer.weight"):
            m = k[:-len("layer.weight")]
            w, s = f(v), f(sd[m + "scale"])
            out[m + "weight"] = (s.reshape(-1, *([1] * (w.dim() - 1))) * w).cpu()
            out[m + "bias"] = (s * f(sd[m + "layer.bias"]) + f(sd[m + "shift"])).cpu()
        elif method == "ssf" and (k.endswith((".layer.bias", ".scale", ".shift"))):
            continue
        else:
            out[k] = v
    return out
