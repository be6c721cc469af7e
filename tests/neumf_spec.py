"""NeuMF restated from its formulas, for the tests (tests/test_neumf_cpu.py,
tests/test_gpu_neumf.py):

    h1(u, i)    = relu(W1 [U_mlp[u] | I_mlp[i]] + b1),  h_l = relu(W_l h_{l-1} + b_l)
    logit(u, i) = w_mf . (U_mf[u] * I_mf[i]) + w_h . h_L + b     (predict_layer = [w_mf | w_h], b)
    loss        = mean BCE(sigmoid(logit), label)

NeuMFRef is a torch module with the reference's module names and construction order
(float32 as built: the seeded-construction test compares it bit for bit; .double() for the
float64 restatement that carries a model's weights, ref_of). The numpy half draws weights
whose logits spread to O(1), evaluates the [users, items] logits in float64, the fp32
split-layer form K14c computes, and the expected masked top-K.
"""
import numpy as np
import torch
import torch.nn as nn


class _Layers(nn.Module):
    """[Dropout -> Linear -> ReLU] per layer under the name mlp_layers.mlp_layers."""

    def __init__(self, sizes, dropout):
        super().__init__()
        mods = []
        for a, b in zip(sizes[:-1], sizes[1:]):
            mods += [nn.Dropout(p=dropout), nn.Linear(a, b), nn.ReLU()]
        self.mlp_layers = nn.Sequential(*mods)

    def forward(self, x):
        return self.mlp_layers(x)


class NeuMFRef(nn.Module):

    def __init__(self, n_users, n_items, dmf, dm, hidden, mf=True, mlp=True, dropout=0.0):
        super().__init__()
        self.mf, self.mlp, self.dmf = mf, mlp, dmf
        self.user_mf_embedding = nn.Embedding(n_users, dmf)
        self.item_mf_embedding = nn.Embedding(n_items, dmf)
        self.user_mlp_embedding = nn.Embedding(n_users, dm)
        self.item_mlp_embedding = nn.Embedding(n_items, dm)
        self.mlp_layers = _Layers([2 * dm] + list(hidden), dropout)
        if mf or mlp:
            self.predict_layer = nn.Linear((dmf if mf else 0) + (hidden[-1] if mlp else 0), 1)
        for m in self.modules():                      # Module.apply's order: children first
            if isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight.data, mean=0.0, std=0.01)

    def logits(self, user, item):
        w, b = self.predict_layer.weight[0], self.predict_layer.bias
        z = b.expand(user.shape[0])
        if self.mf:
            z = z + (w[:self.dmf] * self.user_mf_embedding(user) * self.item_mf_embedding(item)).sum(-1)
        if self.mlp:
            h = torch.cat([self.user_mlp_embedding(user), self.item_mlp_embedding(item)], -1)
            z = z + (w[self.dmf if self.mf else 0:] * self.mlp_layers(h)).sum(-1)
        return z

    def forward(self, user, item):
        return torch.sigmoid(self.logits(user, item))

    def calculate_loss(self, user, item, label):
        p = self.forward(user, item)
        y = label.to(p.dtype)
        return -(y * torch.log(p) + (1 - y) * torch.log(1 - p)).mean()


def ref_of(model):
    """The float64 restatement carrying a NeuMF model's weights."""
    ref = NeuMFRef(model.n_users, model.n_items, model.mf_embedding_size,
                   model.mlp_embedding_size, list(model.mlp_hidden_size), bool(model.mf_train),
                   bool(model.mlp_train)).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in model.state_dict().items()})
    return ref


# ------------------------------------------------------------------ the scorer's numpy half
def draw_weights(seed, n_users, n_items, dmf, dm, hidden):
    """Weights whose logits spread to O(1): embeddings N(0, 1), layer weights
    N(0, 2 / fan_in), biases N(0, 0.1^2), predict N(0, 1 / fan_in); drawn in float64, cast to
    float32 (the values every form below starts from). dmf 0: no MF half."""
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)
    w = {'U_mf': f(rng.standard_normal((n_users, dmf))), 'I_mf': f(rng.standard_normal((n_items, dmf))),
         'U_mlp': f(rng.standard_normal((n_users, dm))), 'I_mlp': f(rng.standard_normal((n_items, dm))),
         'W': [], 'b': []}
    sizes = [2 * dm] + list(hidden)
    for a, b in zip(sizes[:-1], sizes[1:]):
        w['W'].append(f(rng.standard_normal((b, a)) * np.sqrt(2.0 / a)))
        w['b'].append(f(rng.standard_normal(b) * 0.1))
    fan = dmf + hidden[-1]
    w['predict'] = f(rng.standard_normal(fan) / np.sqrt(fan))
    w['bias'] = f(rng.standard_normal(1) * 0.1)
    return w


def logits64(w, users):
    """[len(users), n_items] logits in float64 from the unsplit formula."""
    d = lambda a: np.asarray(a, dtype=np.float64)
    dmf = w['U_mf'].shape[1]
    nq, I = len(users), w['I_mf'].shape[0]
    h = np.concatenate([np.repeat(d(w['U_mlp'])[users], I, axis=0),
                        np.tile(d(w['I_mlp']), (nq, 1))], axis=1)
    for W, b in zip(w['W'], w['b']):
        h = np.maximum(h @ d(W).T + d(b), 0.0)
    z = (h @ d(w['predict'])[dmf:]).reshape(nq, I) + d(w['bias'])[0]
    if dmf:
        z = z + (d(w['U_mf'])[users] * d(w['predict'])[:dmf]) @ d(w['I_mf']).T
    return z


def logits32_split(w, users):
    """The fp32 split-layer form: A = U_mlp W1u^T + b1, Bm = I_mlp W1i^T,
    h1 = relu(A[u] + Bm[i]), layers 2..L, head, MF dot — every step in float32."""
    dmf, dm = w['U_mf'].shape[1], w['U_mlp'].shape[1]
    nq, I = len(users), w['I_mf'].shape[0]
    W1 = w['W'][0]
    A = w['U_mlp'][users] @ W1[:, :dm].T + w['b'][0]
    Bm = w['I_mlp'] @ W1[:, dm:].T
    h = np.maximum(A[:, None, :] + Bm[None, :, :], np.float32(0)).reshape(nq * I, -1)
    for W, b in zip(w['W'][1:], w['b'][1:]):
        h = np.maximum(h @ W.T + b, np.float32(0))
    z = (h @ w['predict'][dmf:]).reshape(nq, I) + w['bias'][0]
    if dmf:
        z = z + (w['U_mf'][users] * w['predict'][:dmf]) @ w['I_mf'].T
    assert z.dtype == np.float32
    return z


def masked_topk(z, hist, K):
    """Per user the K best items by (score desc, id asc) with item 0 and the history
    masked: ids [nq, K] (-1 past the unmasked items) and, per position, the smaller score
    gap to its neighbours in that order (inf where there is no neighbour)."""
    nq, I = z.shape
    ids = np.full((nq, K), -1, dtype=np.int64)
    gap = np.full((nq, K), np.inf)
    for q in range(nq):
        ok = np.ones(I, dtype=bool)
        ok[0] = False
        if hist is not None:
            ok[np.asarray(hist[q], dtype=np.int64)] = False
        cand = np.flatnonzero(ok)
        order = cand[np.lexsort((cand, -z[q, cand]))]
        s = z[q, order]
        n = min(K, len(order))
        ids[q, :n] = order[:n]
        for r in range(n):
            g = np.inf
            if r > 0:
                g = min(g, s[r - 1] - s[r])
            if r + 1 < len(order):
                g = min(g, s[r] - s[r + 1])
            gap[q, r] = g
    return ids, gap


def make_history(seed, nq, I, per_user=20, nearly_all=None):
    """Sorted history lists (items 1..I-1); user `nearly_all` has all but 3 items masked."""
    rng = np.random.default_rng(seed)
    hist = []
    for q in range(nq):
        n = min(per_user, max(I - 2, 0))
        hist.append(sorted(rng.choice(np.arange(1, I), n, replace=False).tolist()) if n else [])
    if nearly_all is not None and I > 4:
        keep = set(rng.choice(np.arange(1, I), 3, replace=False).tolist())
        hist[nearly_all] = [i for i in range(1, I) if i not in keep]
    return hist
