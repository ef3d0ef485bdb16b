"""float64 CPU reference for variable-length histories (per-sample lengths), in the style of tests/adam_ref.py.

Semantics: sample b's leading lengths[b] history slots are valid, the rest is padding; the result for sample b is what the
unmasked encoder gives on x[b, :len] with the first len rows of the (flipped) positional table.  The reference is built
from oracle.cpu_ref pieces BY TRUNCATION, one sample at a time; `encoder_masked` is the vectorised additive-mask form of
the same thing for the one large case (their agreement is a CPU test: tests/test_history_lengths_cpu.py).
Gradients come from torch autograd over these forward formulas, in float64.
"""
import math

import torch

from oracle import cpu_ref as R

F64 = torch.float64


def f64(t):
    return None if t is None else t.detach().to("cpu", F64)


def attention_core(qkv, B, H, D, heads, lengths):
    """The attention core alone on the packed projection qkv [B*H, 3D] = [Q | K | V] -> ctx [B*H, D]; sample b by
    truncation to its first lengths[b] rows, padded rows of ctx = 0.  (The algebra of R.self_attention_layer between its
    two projections; `layer_from_core` below composes it back into that function's result.)"""
    dh = D // heads
    q3 = qkv.reshape(B, H, 3 * D)
    out = []
    for b in range(B):
        n = int(lengths[b])
        t = q3[b, :n]
        q, k, v = (t[:, i * D:(i + 1) * D].reshape(n, heads, dh).permute(1, 0, 2) for i in range(3))
        s = (q * (1.0 / math.sqrt(dh))) @ k.transpose(-1, -2)
        s = s - s.max(dim=-1, keepdim=True).values
        p = torch.exp(s)
        p = p / p.sum(dim=-1, keepdim=True)
        c = (p @ v).permute(1, 0, 2).reshape(n, D)
        out.append(torch.cat([c, c.new_zeros(H - n, D)]))
    return torch.cat(out)


def layer_from_core(x, w_in, b_in, w_out, b_out, heads):
    """R.self_attention_layer rebuilt around attention_core (full lengths): pins the core against the oracle."""
    B, H, D = x.shape
    qkv = x.reshape(B * H, D) @ w_in.t() + b_in
    ctx = attention_core(qkv, B, H, D, heads, [H] * B)
    return (ctx @ w_out.t() + b_out).reshape(B, H, D)


def encoder_truncated(x, lengths, layers, heads, pe):
    """[B, H, D] -> [B, 2, D]: R.history_encoder_forward(x[b:b+1, :len], layers, heads, pe[:len]) per sample."""
    rows = []
    for b in range(x.shape[0]):
        n = int(lengths[b])
        rows.append(R.history_encoder_forward(x[b:b + 1, :n], layers, heads, None if pe is None else pe[:n]))
    return torch.cat(rows)


def encoder_masked(x, lengths, layers, heads, pe):
    """The same by an additive key mask (-inf on padded keys) over the whole batch at once; padded rows of the input are
    zeroed first so that nothing they hold can reach a valid row."""
    B, H, D = x.shape
    dh = D // heads
    lengths = torch.as_tensor(lengths)
    valid = torch.arange(H)[None, :] < lengths[:, None]  # [B, H]
    xv = torch.where(valid[:, :, None], x, torch.zeros_like(x))
    pooled = xv.sum(dim=1) / lengths[:, None].to(x.dtype)
    h = xv if pe is None else torch.where(valid[:, :, None], xv + pe[None], torch.zeros_like(x))
    bias = torch.zeros(B, 1, 1, H, dtype=x.dtype).masked_fill(~valid[:, None, None, :], float("-inf"))
    for w_in, b_in, w_out, b_out in layers:
        qkv = h.reshape(B * H, D) @ w_in.t() + b_in
        q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(B, H, heads, dh).permute(0, 2, 1, 3) for i in range(3))
        s = (q * (1.0 / math.sqrt(dh))) @ k.transpose(-1, -2) + bias
        s = s - s.max(dim=-1, keepdim=True).values
        p = torch.exp(s)
        p = p / p.sum(dim=-1, keepdim=True)
        c = (p @ v).permute(0, 2, 1, 3).reshape(B * H, D)
        h = (c @ w_out.t() + b_out).reshape(B, H, D)
    return torch.stack([h[:, 0, :], pooled], dim=1)


def last_layer_row0(x, lengths, w_in, b_in, w_out, b_out, heads):
    """Row 0 of one attention layer per sample, by truncation: what the collapsed last layer produces.  [B, D]."""
    return torch.cat([R.self_attention_layer(x[b:b + 1, :int(lengths[b])], w_in, b_in, w_out, b_out, heads)[:, 0, :]
                      for b in range(x.shape[0])])


def masked_pool(x, lengths):
    """(x with padded rows zeroed, mean over the valid rows): tt_hist_embed_pool_len without the positional table."""
    B, H, _ = x.shape
    valid = torch.arange(H)[None, :] < torch.as_tensor(lengths)[:, None]
    xv = torch.where(valid[:, :, None], x, torch.zeros_like(x))
    return xv, xv.sum(dim=1) / torch.as_tensor(lengths)[:, None].to(x.dtype)


def user_embedding(params, user_id, user_features, user_history, lengths, heads, pe, masked=False):
    """R.user_embedding with the history summary taken by truncation (ref:...with_user_history_encoder.py:85-122)."""
    id_emb = params["user_id_embedding_arch.weight"][user_id]
    feat = R.feature_mlp(user_features, params, "user_features_arch.")
    hist = params["item_id_embedding_arch.weight"][user_history]
    enc = encoder_masked if masked else encoder_truncated
    summary = enc(hist, lengths, R.encoder_layers_from_params(params), heads, pe)
    tin = torch.cat([id_emb, feat, summary.reshape(summary.shape[0], -1)], dim=1)
    return tin @ params["user_tower_arch.weight"].t() + params["user_tower_arch.bias"]


def train_forward(params, batch, lengths, uvw, heads, pe, debias=R.debias_identity):
    """R.train_forward of the history model with per-sample lengths."""
    user_id, user_features, user_history, item_id, item_features, position, labels = batch
    u = user_embedding(params, user_id, user_features, user_history, lengths, heads, pe)
    it = R.item_embeddings(params, item_id, item_features)
    return R.training_loss(u, it, position, labels, uvw, params, debias)


def loss_and_grads(params, batch, lengths, uvw, heads, pe, debias=R.debias_identity):
    """(loss, {name: gradient}) in float64; `params` / `batch` in any precision."""
    leaves = {k: f64(v).requires_grad_(True) for k, v in params.items()}
    b = [t.detach().cpu() if not t.is_floating_point() else f64(t) for t in batch]
    loss = train_forward(leaves, b, lengths, f64(uvw), heads, f64(pe), debias)
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return loss.detach(), {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(leaves, grads)}
