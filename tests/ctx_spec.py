"""Float64 restatement of the context-field operation K8 computes (include/mirec.h, K8;
reference abstract_recommender.py:199-412, layers.py:121-171 and :1029-1062,
deepfm.py:58-70), in plain differentiable torch ops, with the magnitude of every output.

fields(tables, cols, layout) -> (concat [B, F, d], y [B]):
  token rows T[id + offset]; token_seq masked means sum(mask * e) / (count + 1e-8) with
  masked first-order sums; float rows Ef[j] * x; concat order token | token_seq | float;
  y = ((float + token) + seq) + bias [+ 0.5 * sum_k((sum_f e)^2 - sum_f e^2) with fm].

mag: the same formula with |.| on every table entry and float value and `+` in place of
`-`: the sum of the absolute values of the terms that enter an output. reference() gives
it for y, every concat element and every dense table-gradient entry (the gradient of
|g_concat| . concat + |g_y| . y through the |.| formula is the |.| sum of the backward's
terms, scatter included). Tolerances of the GPU tests are stated against it: FM's
S^2 - Q and the scatter sums cancel, so an output can be near 0 with terms of O(10).

Also here, shared by the CPU and GPU tests: the case generator (make_case), the float32
restatement of y in field order (y_float32) and the sigmoid + BCE point sets."""
import numpy as np
import torch

TABLE_KEYS = ('T', 'T1', 'Ef', 'Ef1', 'bias')


class Layout:
    """The field lists fields() reads (recbole_amd.model.context.FieldLayout has them too)."""

    def __init__(self, token_names, seq_names, float_names, token_offsets):
        self.token_names, self.seq_names = list(token_names), list(seq_names)
        self.float_names = list(float_names)
        self.token_offsets = [int(x) for x in token_offsets]
        self.n_fields = len(self.token_names) + len(self.seq_names) + len(self.float_names)


def fields(tables, cols, layout, fm=True, mag=False):
    """tables: T [V, d], T1 [V, 1], Ef [nf, d], Ef1 [nf, 1], bias [1], seq / seq1 (lists of
    [V_i, d] / [V_i, 1]) as float64 tensors (None / [] where the kind has no field); cols:
    name -> ids [B] / [B, L] (int64) or values [B]. mag=True: the magnitude form."""
    a = (lambda t: t.abs()) if mag else (lambda t: t)
    parts, fo_tok, fo_seq, fo_float = [], 0.0, 0.0, 0.0
    for name, off in zip(layout.token_names, layout.token_offsets):
        rows = cols[name].long() + off
        parts.append(a(tables['T'])[rows].unsqueeze(1))
        fo_tok = fo_tok + a(tables['T1'])[rows, 0]
    for i, name in enumerate(layout.seq_names):
        ids = cols[name].long()
        mask = (ids != 0).to(torch.float64)
        e = a(tables['seq'][i])[ids] * mask.unsqueeze(2)
        parts.append((e.sum(1) / (mask.sum(1, keepdim=True) + 1e-8)).unsqueeze(1))
        fo_seq = fo_seq + (a(tables['seq1'][i])[ids, 0] * mask).sum(1)
    for j, name in enumerate(layout.float_names):
        x = a(cols[name].to(torch.float64))
        parts.append((a(tables['Ef'])[j].unsqueeze(0) * x.unsqueeze(1)).unsqueeze(1))
        fo_float = fo_float + a(tables['Ef1'])[j, 0] * x
    concat = torch.cat(parts, dim=1)
    y = ((fo_float + fo_tok) + fo_seq) + a(tables['bias'])[0]
    if fm:
        S, Q = concat.sum(1), (concat * concat).sum(1)
        y = y + 0.5 * ((S * S + Q) if mag else (S * S - Q)).sum(1)
    return concat, y + torch.zeros(concat.shape[0], dtype=torch.float64)


def _leaves(tables, absolute=False):
    f = lambda t: (t.detach().double().abs() if absolute else t.detach().double()
                   ).clone().requires_grad_(True)
    out = {k: (None if tables.get(k) is None else f(tables[k])) for k in TABLE_KEYS}
    out['seq'] = [f(t) for t in tables.get('seq', [])]
    out['seq1'] = [f(t) for t in tables.get('seq1', [])]
    return out


def _flat(tables):
    out = {k: tables[k] for k in TABLE_KEYS if tables.get(k) is not None}
    for i, (s, s1) in enumerate(zip(tables['seq'], tables['seq1'])):
        out[f'seq{i}'], out[f'seq1_{i}'] = s, s1
    return out


def reference(tables, cols, layout, g_concat=None, g_y=None, fm=True):
    """(ref, mag): dicts with 'concat', 'y' and, when g_y is given, 'd<table>' for every
    table in _flat's naming (dT, dT1, dEf, dEf1, dbias, dseq0, dseq1_0, ...) — the float64
    values and their magnitudes. g_concat None: zero."""
    out = []
    for absolute in (False, True):
        lv = _leaves(tables, absolute)
        concat, y = fields(lv, cols, layout, fm=fm, mag=absolute)
        res = {'concat': concat.detach(), 'y': y.detach()}
        if g_y is not None:
            gy = g_y.detach().double().cpu()
            gc = torch.zeros_like(concat) if g_concat is None else \
                g_concat.detach().double().cpu().reshape(concat.shape)
            if absolute:
                gy, gc = gy.abs(), gc.abs()
            flat = _flat(lv)
            grads = torch.autograd.grad((concat * gc).sum() + (y * gy).sum(),
                                        list(flat.values()), allow_unused=True)
            for k, g in zip(flat, grads):
                res['d' + k] = torch.zeros_like(flat[k]) if g is None else g
        out.append(res)
    return out[0], out[1]


def contribution_grad(tables, cols, layout, g_y, fm=True):
    """dL/d concat [B, F, d] for L = g_y . y: the backward's ge with g_concat = 0."""
    lv = _leaves(tables)
    concat, y = fields(lv, cols, layout, fm=fm)
    if not fm:
        return torch.zeros_like(concat).detach()
    return torch.autograd.grad((y * g_y.detach().double().cpu()).sum(), concat)[0]


# ------------------------------------------------------------------ cases
def make_case(d, B, nt, ns, nf, seed, integer=False):
    """float32 CPU tables, columns and layout of one case. Token vocabularies of 2-50 rows
    per field; ids include 0, each field's last row and repeats; token_seq lengths 1 and 5
    with all-zero rows, full rows and a zero in the middle. integer: every table entry,
    float value and the bias an integer in [-3, 3] (float32 sums are then exact)."""
    g = torch.Generator().manual_seed(seed)
    if integer:
        val = lambda *s: torch.randint(-3, 4, s, generator=g).to(torch.float32)
    else:
        val = lambda *s: torch.randn(*s, generator=g)
    cols, tables = {}, {'T': None, 'T1': None, 'Ef': None, 'Ef1': None, 'seq': [], 'seq1': []}
    dims = [int(torch.randint(2, 51, (1,), generator=g)) for _ in range(nt)]
    if nt:
        dims[0] = 2
        dims[-1] = 50 if nt > 1 else 2
        V = sum(dims)
        tables['T'], tables['T1'] = val(V, d), val(V, 1)
    for i, n in enumerate(dims):
        ids = torch.randint(0, n, (B,), generator=g)
        ids[0] = 0
        ids[-1] = n - 1
        if B > 2:
            ids[B // 2] = n - 1          # a repeat of the last row
        cols[f'tok{i}'] = ids
    for i in range(ns):
        L, n = (1, 5)[i % 2], (7, 23)[i % 2]
        ids = torch.randint(1, n, (B, L), generator=g)
        ids[0::4] = 0                     # count 0: e = 0 and its gradients 0
        if L > 2:
            ids[1::4, L // 2] = 0         # a zero in the middle
            ids[2::4, L - 1] = n - 1      # full rows that hit the last row
        cols[f'seq{i}'] = ids
        tables['seq'].append(val(n, d))
        tables['seq1'].append(val(n, 1))
    if nf:
        tables['Ef'], tables['Ef1'] = val(nf, d), val(nf, 1)
    for j in range(nf):
        cols[f'flt{j}'] = val(B)
    tables['bias'] = val(1)
    offsets = np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(np.int64) if nt else []
    layout = Layout([f'tok{i}' for i in range(nt)], [f'seq{i}' for i in range(ns)],
                    [f'flt{j}' for j in range(nf)], offsets)
    return tables, cols, layout


WIDTHS = (1, 3, 4, 5, 8, 10, 16, 17, 32, 33, 64)
FIELD_SETS = ((3, 1, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (8, 0, 0), (9, 0, 0), (5, 2, 10))


def tolerance_cases():
    """(d, B, (nt, ns, nf)) of every float64-tolerance case of tests/test_gpu_context.py."""
    out = [(d, 257, fs) for d in WIDTHS for fs in ((3, 1, 2), (5, 2, 10))]
    out += [(10, 257, fs) for fs in FIELD_SETS if fs not in ((3, 1, 2), (5, 2, 10))]
    out += [(d, B, (3, 1, 2)) for d in (4, 10, 64) for B in (1, 37)]
    return out


def case_seed(d, B, fs):
    return 1000 * d + 7 * B + 100 * fs[0] + 10 * fs[1] + fs[2]


def y_float32(tables, cols, layout, fm=True):
    """y in plain float32 numpy: every sum one float32 add at a time, fields in concat
    order, columns in column order."""
    f32 = np.float32
    np_ = lambda t: t.detach().cpu().numpy()
    B = len(next(iter(cols.values())))
    d = next(t for t in (tables['T'], tables['Ef'], *tables['seq']) if t is not None).shape[1]
    rows = []                       # (kind, e [B, d], w1 [B]) per field
    for name, off in zip(layout.token_names, layout.token_offsets):
        r = np_(cols[name]) + off
        rows.append((0, np_(tables['T'])[r], np_(tables['T1'])[r, 0]))
    for i, name in enumerate(layout.seq_names):
        ids = np_(cols[name])
        s, w, cnt = np.zeros((B, d), f32), np.zeros(B, f32), np.zeros(B, f32)
        for t in range(ids.shape[1]):
            m = (ids[:, t] != 0).astype(f32)
            s = s + np_(tables['seq'][i])[ids[:, t]] * m[:, None]
            w = w + np_(tables['seq1'][i])[ids[:, t], 0] * m
            cnt = cnt + m
        rows.append((1, s / (cnt + f32(1e-8))[:, None], w))
    for j, name in enumerate(layout.float_names):
        x = np_(cols[name]).astype(f32)
        rows.append((2, np_(tables['Ef'])[j][None, :] * x[:, None], np_(tables['Ef1'])[j, 0] * x))
    fo = [np.zeros(B, f32) for _ in range(3)]
    S, Q = np.zeros((B, d), f32), np.zeros((B, d), f32)
    for kind, e, w in rows:
        fo[kind] = fo[kind] + w
        S, Q = S + e, Q + e * e
    y = ((fo[2] + fo[0]) + fo[1]) + np_(tables['bias'])[0]
    if fm:
        t, acc = S * S - Q, np.zeros(B, f32)
        for k in range(d):
            acc = acc + t[:, k]
        y = y + f32(0.5) * acc
    assert y.dtype == f32
    return y


def float32_ratio():
    """The largest |y_float32 - y_float64| / mag over tolerance_cases(), both forms."""
    worst = 0.0
    for d, B, fs in tolerance_cases():
        tables, cols, layout = make_case(d, B, *fs, seed=case_seed(d, B, fs))
        for fm in (True, False):
            ref, mag = reference(tables, cols, layout, fm=fm)
            err = np.abs(y_float32(tables, cols, layout, fm).astype(np.float64) - ref['y'].numpy())
            worst = max(worst, float((err / mag['y'].numpy()).max()))
    return worst


# ------------------------------------------------------------------ sigmoid + BCE points
BCE_RTOL, BCE_ATOL = 1e-4, 2.4e-7          # moderate set against float64 (2 ulps of 1.0)
BCE_Z_SATURATED = (20., -20., 30., -30., 95., -95., 200., -200.)


def bce_moderate(B, seed):
    """z uniform in [-6, 6] (torch-float32 itself is 3e-5 off float64 at |z| <= 6 and
    2e-4 at |z| <= 8: p rounds near 1), t in {0, 1}."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.rand(B, generator=g) * 12 - 6).to(torch.float32)
    t = torch.randint(0, 2, (B,), generator=g).to(torch.float32)
    return z, t


def bce_saturated():
    z = torch.tensor([v for v in BCE_Z_SATURATED for _ in (0, 1)], dtype=torch.float32)
    t = torch.tensor([0., 1.] * len(BCE_Z_SATURATED), dtype=torch.float32)
    return z, t


def bce_torch(z, t, dtype, grad_scale=1.0):
    """(p, loss_b, dz) of BCELoss(reduction='none')(sigmoid(z), t) on the CPU in `dtype`,
    dz by autograd for L = grad_scale * sum(loss_b)."""
    zz = z.detach().cpu().to(dtype).clone().requires_grad_(True)
    p = torch.sigmoid(zz)
    loss = torch.nn.BCELoss(reduction='none')(p, t.detach().cpu().to(dtype))
    (loss.sum() * grad_scale).backward()
    return p.detach(), loss.detach(), zz.grad
