"""Per-configuration measurements of the model rows of SURVEY.md §8 beyond the
C2 headline (bench.py): one JSON line per configuration, 1 GPU.

  C3  SASRec, Amazon-Books shape: I = 3,000,000 (+PAD), L = 50, d = 128, 2 layers,
      2 heads, inner 256, 100 uniform negatives per sequence from the device walk
      (RepeatableSampler, K4), sampled-softmax loss (K9b), dense Adam over every
      parameter (the reference's optim.Adam on nn.Embedding(sparse=False)).
      Unit: sequences/s; dominant-kernel rooflines from HIP events.
      --c3-loss CE-library / CE-fused: the same step with the reference's default
      full-catalogue cross entropy (no negatives drawn), on the library GEMM path or on
      K12 (ce_kernel='fused'); the record carries the peak allocated memory.
      --c3-model GRU4Rec: the same batches and item table through GRU4Rec at the
      reference's default widths (E = 64, H = 128), run eagerly (the model does not
      offer its step for capture); GRU4Rec has no sampled softmax, so the default loss there is BPR with one
      walk negative per sequence (--c3-loss CE-library / CE-fused as for SASRec).
  C4  DeepFM, Criteo shape: 13 float + 26 token fields, vocabularies summing to
      33,000,000 (10M, 8M, 5M, 4M, 3M, then geometric down to 3), Zipf(1.1) ids,
      d = 16, MLP 624-128-128-128-1 (dropout 0.2), BCE, B = 2,048, dense Adam.
      Unit: samples/s.
  C5  LightGCN, 10M users x 5M items, 100M edges (Zipf items, Zipf-like user
      degrees), d = 256, 2 layers: propagation (K7) once, then full-sort top-10
      (K6) of a bounded sample of users against all 5M items. Unit: users/s.
  N2  NeuMF at C2's table shape (138,494 x 26,745 rows, widths 64 / 64 / [128, 64, 32]):
      the pointwise train step (samples/s), the fused full-sort evaluation (K14c, users/s,
      share of the fp32 MFMA peak) and the generic fallback on a user subset. Not in the
      default --configs list: --configs N2.
  A2  MultiVAE at C2's table shape and interaction count (synthetic Zipf histories, default
      widths 600 / 128, B = 2,048 users): the K15 train step against a dense fp32 torch
      statement of the reference's step on the same device, weights and batches (ms/step,
      users/s, peak allocated), and the full-sort evaluation, fused (K15d) against the
      generic sequence on a user subset. Not in the default list: --configs A2.
  G2  NGCF on C5's graph generator at --scale (widths 64 / [64, 64, 64], message dropout
      0.1, B = 2,048 BPR triples): one training step on K7 + K16 + K3 against a torch
      statement of the same step (torch.sparse.mm, Linear, leaky_relu, dropout, normalize,
      cat, gathers) on the same device, weights and batches: ms/step and peak allocated of
      both over alternating timed windows, and the two steps' loss and gradients compared
      with the dropout off. Not in the default list: --configs G2.
  B3  BERT4Rec: 65,536 items + PAD, L = 50, d = 128, 2 layers, 2 heads, B = 1,024,
      mask_ratio 0.2 (M = 10), loss 'CE', run eagerly: steps/s with ce_kernel 'fused'
      (K17b + K12 over the masked rows + K17c) and 'library' (the reference's op sequence,
      a [B, M, n_items] logits tensor), the peak allocated memory of both, K17a alone (HIP
      events) and the wall time of the reference's host masking loop restated here in pure
      Python on the same batch. Not in the default list: --configs B3.
  X4  xDeepFM at the C4 shape (13 float + 26 token fields, V = 33 M, d = 16) with the
      reference's defaults (CIN [100, 100, 100], direct False, MLP 128-128-128-1, dropout
      0.2, reg_weight 5e-4), B = 2,048: the training step with cin_kernel 'fused' (K18)
      against 'library' (einsum + conv1d, z [B, H m, D] in memory) on copies of the same
      weights and batches, alternating windows, peak memory of both, K18's three kernels'
      launch times and MFMA fractions. Not in the default list: --configs xDeepFM (or X4).
  D4  DCN at the same C4 shape (n = 39 x 16 = 624) with the reference's defaults (6 cross
      layers, MLP 256-256-256 with BatchNorm, dropout 0.2, reg_weight 2), B = 2,048: the
      training step with cross_kernel 'fused' (K19, head mode) against 'library' (the
      reference's op sequence, cat, predict_layer) on copies of the same weights and batches,
      alternating windows, peak memory of both, K19's two launch times. Not in the default
      list: --configs DCN (or D4).
  A4  AFM at the same C4 field shape (F = 39, P = 741 pairs) with the reference's defaults
      (attention_size 25, dropout 0.3, reg_weight 2) and d = 16, B = 2,048: the training step
      with afm_kernel 'fused' (K20) against 'library' (the reference's op sequence, the
      [B, P, d] and [B, P, A] pair tensors in memory) on copies of the same weights and
      batches, alternating windows, each side's peak memory above what was resident, K20's
      two launch times. Not in the default list: --configs AFM (or A4).

Synthetic data (seeded numpy PCG64 / torch generators), random init. Each step is
the Trainer's generic step: zero_grad -> calculate_loss -> backward -> FusedAdam.
Usage: python tools/bench_models.py [--configs C3,C4,C5] [--steps K] [--warmup W]
       [--scale S] (S < 1 shrinks the tables / graph for a quick run).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F32_PEAK_TFLOPS = 157.3   # fp32 matrix peak (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md
FP32_PEAK_TFLOPS = 157.3   # fp32 MFMA / vector peak
CPU_BASELINE = True
ADAM_MODE = 'deferred'
GRAPH_STEP = True


class StubDataset:
    """The dataset surface a model constructor reads (fields / field2type / num)."""

    def __init__(self, types, nums, uid=None, iid=None):
        self.field2type = dict(types)
        self._num = dict(nums)
        self.uid_field, self.iid_field = uid, iid

    def fields(self, ftype=None, source=None):
        return [f for f in self.field2type if ftype is None or self.field2type[f] in ftype]

    def num(self, field):
        return self._num[field]


MARKERS = os.environ.get('MODELS_MARKERS') == '1'   # trace markers (tools/step_breakdown.py)


def _timed(fn, steps, warmup, opt=None):
    """Mean wall time per step over `steps` steps; with a deferred optimizer the
    flush that completes every row is inside the timed region (no work skipped).
    MODELS_MARKERS=1: two 1-cycle spin kernels bracket the timed region in a kernel
    trace (tools/step_breakdown.py)."""
    for _ in range(warmup):
        fn()
    if opt is not None:
        opt.flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if MARKERS:
        torch.cuda._sleep(1)
    for _ in range(steps):
        fn()
    if opt is not None:
        opt.flush()
    if MARKERS:
        torch.cuda._sleep(1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _window_events(step, names, steps=8):
    """HIP events around the named native launches (ops.timed_launch) over `steps`
    eager steps enqueued behind a spin kernel (the host enqueues the whole window
    before the GPU reaches it, so an event pair brackets its kernel only). Returns
    {name: (launches per step, mean launch us)}."""
    from recbole_amd import ops
    ops.KERNEL_EVENTS = {n: [] for n in names}
    try:
        torch.cuda.synchronize()
        torch.cuda._sleep(int(2.4e3 * 1500 * steps))
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ev = ops.KERNEL_EVENTS
    finally:
        ops.KERNEL_EVENTS = None
    return {n: (len(v) / steps, float(np.mean([a.elapsed_time(b) * 1e3 for a, b in v])))
            for n, v in ev.items() if v}


def _pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` (a name, or a tuple of names whose per-launch
    traffic is summed: one call's launches) from the newest committed models PMC summary
    (profiles/r*_models_pmc.json, tools/models_pmc.py), or None when that summary did not
    trace every one of them (never an older file's entry for a kernel the step no longer
    runs)."""
    import glob
    import json
    paths = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_models_pmc.json')))
    if not paths:
        return None, None
    recs = json.load(open(paths[-1]))
    names = (kernel,) if isinstance(kernel, str) else tuple(kernel)
    got = [recs.get(k) for k in names]
    if any(r is None for r in got):
        return None, None
    return sum(r['traffic'] for r in got), os.path.basename(paths[-1])


def _step_breakdown(config):
    """The committed per-step kernel breakdown of the timed step (rocprofv3 kernel
    trace, tools/step_breakdown.py): profiles/r*_<config>_step.json, newest."""
    import glob
    import json
    paths = sorted(glob.glob(os.path.join(ROOT, 'profiles', f'r*_{config}_step.json')))
    if not paths:
        return None
    r = json.load(open(paths[-1]))
    return {'source': os.path.basename(paths[-1]), 'wall_us_per_step': r['wall_us_per_step'],
            'kernel_us_per_step': r['kernel_us_per_step'],
            'launches_per_step': r['launches_per_step'], 'dominant': r['dominant'],
            'top5': [{k: x[k] for k in ('kernel', 'us_per_step', 'launches_per_step')}
                     for x in r['kernels'][:5]]}


def _event_time(fn, reps=10):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def _zipf_ids(rng, a, n, vmax):
    """Zipf(a) ranks clipped to [1, vmax] (id 0 is [PAD])."""
    return np.minimum(rng.zipf(a, n), vmax).astype(np.int64)


# ----------------------------------------------------------------------------- C4
def c4_vocab(total=33_000_000):
    big = [10_000_000, 8_000_000, 5_000_000, 4_000_000, 3_000_000]
    rest = total - sum(big)
    r = 0.55
    w = r ** np.arange(21)
    sizes = np.maximum(np.round(w / w.sum() * rest).astype(np.int64), 3)
    sizes[0] += rest - sizes.sum()
    return big + sizes.tolist()


def bench_c4(dev, steps, warmup, scale=1.0, B=2048, d=16, n_batches=16):
    from recbole_amd.config import Config
    from recbole_amd.model.context_aware_recommender import DeepFM
    from recbole_amd.model.context import _CtxFMFn
    from recbole_amd.trainer.optim import FusedAdam
    from recbole_amd.data.interaction import Interaction
    from recbole_amd.utils import FeatureType
    vocab = [max(3, int(v * scale)) for v in c4_vocab()]
    types = {'label': FeatureType.FLOAT}
    nums = {'label': 1}
    for j in range(13):
        types[f'I{j}'], nums[f'I{j}'] = FeatureType.FLOAT, 1
    for j, v in enumerate(vocab):
        types[f'C{j}'], nums[f'C{j}'] = FeatureType.TOKEN, v + 1      # + [PAD]
    config = Config(model='DeepFM', dataset='criteo-synth', config_dict={
        'embedding_size': d, 'load_col': None, 'state': 'ERROR', 'data_path': ROOT})
    config['device'] = dev
    torch.manual_seed(2020)
    model = DeepFM(config, StubDataset(types, nums)).to(dev)
    rng = np.random.default_rng(2020)
    batches = []
    for _ in range(n_batches):
        cols = {'label': torch.as_tensor((rng.random(B) < 0.256).astype(np.float32))}
        for j in range(13):
            x = rng.lognormal(0.0, 2.0, B)
            cols[f'I{j}'] = torch.as_tensor(((x - x.min()) / (x.max() - x.min())).astype(
                np.float32))
        for j, v in enumerate(vocab):
            cols[f'C{j}'] = torch.as_tensor(_zipf_ids(rng, 1.1, B, v))
        batches.append(Interaction(cols).to(dev))
    opt = FusedAdam(model.parameters(), lr=1e-3)
    if ADAM_MODE == 'deferred':
        opt.enable_deferred(model.deferred_tables())
    it = [0]
    gs = None
    if GRAPH_STEP:                 # the Trainer's captured step (trainer/graph_step.py)
        from recbole_amd.trainer.graph_step import GraphedTrainStep
        gs = GraphedTrainStep(model, opt)

    def step():
        b = batches[it[0] % n_batches]
        it[0] += 1
        if gs is not None:
            gs.step(b)
            return
        opt.zero_grad()
        loss = model.calculate_loss(b)
        loss.backward()
        opt.step()

    t = _timed(step, steps, warmup, opt)
    V = sum(nums[f'C{j}'] for j in range(26))
    # the timed step's dominant kernel (profiles/r03_C4_step.json: ctx_fm_bwd_kernel, K8
    # backward), timed live on its stream over eager steps of the same batches.
    # Algorithmic bytes per launch: concat + g_concat read (39 fields x d floats per
    # sample), g_fm read, gradient rows written (26 token + 13 float fields x d floats)
    # and the first-order gradients (39 floats) per sample.
    def eager():
        b = batches[it[0] % n_batches]
        it[0] += 1
        opt.zero_grad()
        model.calculate_loss(b).backward()
        opt.step()
    ev = _window_events(eager, ('ctx_fm_bwd', 'ctx_fm_fwd', 'mlp_fwd', 'mlp_bwd', 'k2_blocks'))
    opt.flush()
    bwd_n, bwd_us = ev['ctx_fm_bwd']
    fwd_n, fwd_us = ev['ctx_fm_fwd']
    # K10 (the MLP on fp32 MFMA): 2 FLOPs per multiply-add of every layer, per launch
    dims = [39 * d, 128, 128, 128, 1]
    mlp_flops = 2 * B * sum(a * b_ for a, b_ in zip(dims[:-1], dims[1:]))
    mf_n, mf_us = ev['mlp_fwd']
    mb_n, mb_us = ev['mlp_bwd']
    k2_n, k2_us = ev['k2_blocks']
    nk = 26 * B                                 # token keys of a step
    k2_bytes = nk * (8 + 4 + 4 + 4)             # keys read; perm, uniq, seg written
    bwd_bytes = B * (2 * 39 * d * 4 + 4 + 39 * d * 4 + 39 * 4)
    fwd_bytes = B * (26 * (d * 4 + 4 + 8) + 13 * 4 + 39 * d * 4 + 4 + 26 * 8)
    traffic, tsrc = _pmc_traffic('ctx_fm_bwd_kernel')
    cpu = None
    if CPU_BASELINE:
        from oracle import cpu_baseline as cb
        thr, how = cb.host_threads()
        runs = [cb.time_deepfm_steps(batches, [f'C{j}' for j in range(26)],
                                     [nums[f'C{j}'] for j in range(26)],
                                     [f'I{j}' for j in range(13)], d, [128, 128, 128],
                                     steps=20, warmup=2, threads=thr) for _ in range(3)]
        sps, used = float(np.median([r[0] for r in runs])), runs[0][2]
        vals = np.array([r[0] for r in runs])
        cpu = {'value': round(sps, 1), 'unit': 'samples/s', 'cores': used, 'kind': 'port',
               'threads_derivation': how, 'runs': [round(r[0], 1) for r in runs],
               'cv': round(float(vals.std() / vals.mean()), 4),
               'sample': f'median of 3 runs of 2 warm-up + 20 timed C4 steps of the oracle '
                         f'restatement on torch CPU (DeepFMCPU + dense optim.Adam over every '
                         f'table), {sum(r[1] for r in runs):.1f} s timed in all; bounded below '
                         f'the 20 + 200 of SURVEY.md 8d: a CPU step moves the 2.1 GB tables '
                         f'several times (~1 s), and the run-to-run spread (cv) is reported'}
    fwd_k = ('mlp_l0_fwd_kernel', 'mlp_fwd_kernel')
    wide = os.environ.get('MIREC_MLP_WIDE_FWD') == '1'       # csrc/mlp.hip wide_fwd_on
    k10 = {'kernel': ('mlp_l0_fwd_kernel + mlp_fwd_kernel (K10 forward: the wide layer 0 over '
                      'the whole chip, then layers 1.. + deep_predict_layer; dropout, ReLU; '
                      'one event pair around both launches)') if wide else
                     ('mlp_fwd_kernel (K10 forward: every layer + deep_predict_layer in one '
                      'launch, one 16-row block per CU; dropout, ReLU)'), 'bound': 'mfma',
           'achieved': round(mlp_flops / (mf_us * 1e-6) / 1e12, 2),
           'peak': MFMA_F32_PEAK_TFLOPS, 'unit': 'TFLOP/s',
           'frac': round(mlp_flops / (mf_us * 1e-6) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
           'traffic': _pmc_traffic(fwd_k)[0],
           'traffic_source': _pmc_traffic(fwd_k)[1],
           'flops_per_launch': mlp_flops, 'launch_us': round(mf_us, 2),
           'launches_per_step': mf_n,
           'timing': 'HIP events around each launch on its stream, 8 eager steps'}
    k2 = {'kernel': 'segsort_radix8_kernel (K2 grouping of the 26 token fields: one chained '
                    'launch, keys formed from the field columns; latency-bound)',
          'bound': 'hbm', 'achieved': round(k2_bytes / (k2_us * 1e-6) / 1e9, 1),
          'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
          'frac': round(k2_bytes / (k2_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 5),
          'traffic': _pmc_traffic('segsort_radix8_kernel')[0],
          'traffic_source': _pmc_traffic('segsort_radix8_kernel')[1],
          'bytes_per_launch': k2_bytes, 'launch_us': round(k2_us, 2), 'launches_per_step': k2_n,
          'timing': 'HIP events around each call on its stream, 8 eager steps'}
    # the roofline of the timed step's dominant kernel (committed trace breakdown)
    sb = _step_breakdown('C4')
    dom = (sb or {}).get('dominant', {}).get('kernel', '') if sb else ''
    roof = k2 if 'segsort' in dom else k10
    return {
        'cpu_baseline': cpu,
        'adam_mode': ADAM_MODE, 'graph_step': bool(GRAPH_STEP),
        'config': 'C4', 'metric': 'train samples/s', 'value': round(B / t, 1),
        'unit': 'samples/s', 'ms_per_step': round(t * 1e3, 3), 'batch': B, 'steps': steps,
        'workload': f'DeepFM Criteo-shape: 13 float + 26 token fields, vocab {V:,} '
                    f'(incl. PADs), d={d}, MLP 624-128-128-128-1, dropout 0.2, BCE, dense Adam',
        'dtype': 'fp32', 'data': 'synthetic (Zipf(1.1) ids, log-normal floats, seeded)',
        'step_breakdown': _step_breakdown('C4'),
        'roofline': roof,
        'k10_fwd': k10,
        'k2_grouping': k2,
        'k10_bwd': {'kernel': 'mlp_bwd_data_kernel + mlp_bwd_wide_kernel (K10 backward: layers '
                              'L-1..1 in row blocks, then layer 0\'s data gradient and every '
                              'weight gradient over the whole chip; one event pair around both '
                              'launches)', 'bound': 'mfma',
                    'traffic': _pmc_traffic(('mlp_bwd_data_kernel', 'mlp_bwd_wide_kernel'))[0],
                    'achieved': round(2 * mlp_flops / (mb_us * 1e-6) / 1e12, 2),
                    'peak': MFMA_F32_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                    'frac': round(2 * mlp_flops / (mb_us * 1e-6) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                    'flops_per_call': 2 * mlp_flops, 'call_us': round(mb_us, 2)},
        'k8_bwd': {'kernel': 'ctx_fm_bwd_kernel<16> (K8 backward)', 'bound': 'hbm',
                     'achieved': round(bwd_bytes / (bwd_us * 1e-6) / 1e9, 1),
                     'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                     'frac': round(bwd_bytes / (bwd_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                     'traffic': traffic, 'traffic_source': tsrc,
                     'bytes_per_launch': bwd_bytes, 'launch_us': round(bwd_us, 2),
                     'launches_per_step': bwd_n,
                     'timing': 'HIP events around each launch on its stream, 8 eager steps'},
        'k8_fwd': {'kernel': 'ctx_fm_fwd_kernel<16> (K8 forward: field gather + first order + '
                             'FM)', 'bound': 'hbm',
                   'achieved': round(fwd_bytes / (fwd_us * 1e-6) / 1e9, 1),
                   'unit': 'GB/s', 'bytes_per_launch': fwd_bytes, 'launch_us': round(fwd_us, 2),
                   'launches_per_step': fwd_n},
    }


# ----------------------------------------------------------------------------- C3
C3_LOSSES = ('SSM', 'CE-library', 'CE-fused')


def bench_c3(dev, steps, warmup, scale=1.0, B=2048, L=50, d=128, n_neg=100, n_batches=8,
             loss='SSM'):
    if loss not in C3_LOSSES:
        raise ValueError(f'loss must be one of {C3_LOSSES}')
    ce = loss != 'SSM'
    from recbole_amd import ops
    from recbole_amd.config import Config
    from recbole_amd.data.interaction import Interaction
    from recbole_amd.model.sequential_recommender import SASRec
    from recbole_amd.trainer.optim import FusedAdam
    from recbole_amd.utils import FeatureType
    n_items = max(1000, int(3_000_000 * scale)) + 1
    config = Config(model='SASRec', dataset='books-synth', config_dict={
        'hidden_size': d, 'inner_size': 256, 'n_layers': 2, 'n_heads': 2,
        'MAX_ITEM_LIST_LENGTH': L, 'loss_type': 'CE' if ce else 'SSM',
        'training_neg_sample_num': 0 if ce else n_neg,
        'ce_kernel': {'CE-library': 'library', 'CE-fused': 'fused'}.get(loss),
        'state': 'ERROR', 'data_path': ROOT})
    config['device'] = dev
    torch.manual_seed(2020)
    model = SASRec(config, StubDataset({'item_id': FeatureType.TOKEN},
                                       {'item_id': n_items})).to(dev)
    rng = np.random.default_rng(2020)
    batches = []
    for _ in range(n_batches):
        lens = np.minimum(rng.poisson(20, B) + 4, L).astype(np.int64)
        seq = np.zeros((B, L), dtype=np.int64)
        ids = _zipf_ids(rng, 1.1, int(lens.sum()), n_items - 1)
        mask = np.arange(L)[None, :] < lens[:, None]
        seq[mask] = ids
        batches.append(Interaction({
            'item_id_list': torch.as_tensor(seq), 'item_length': torch.as_tensor(lens),
            'item_id': torch.as_tensor(_zipf_ids(rng, 1.1, B, n_items - 1)),
            'user_id': torch.as_tensor(rng.integers(1, 1_000_000, B))}).to(dev))
    random_list = torch.as_tensor(rng.permutation(np.arange(1, n_items)).astype(np.int32),
                                  device=dev)
    pr = torch.zeros(1, dtype=torch.int64, device=dev)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    if ADAM_MODE == 'deferred':
        opt.enable_deferred(model.deferred_tables())
    it = [0]
    gs = None
    if GRAPH_STEP:                 # the Trainer's captured step (trainer/graph_step.py)
        from recbole_amd.trainer.graph_step import GraphedTrainStep
        gs = GraphedTrainStep(model, opt)

    def step():
        b = batches[it[0] % n_batches]
        it[0] += 1
        if not ce:
            # the data side (the loader's K4 walk of 100 negatives per sequence) stays eager
            neg = ops.sample_walk(random_list, pr, b['user_id'], n_neg, None, None, 1_000_000,
                                  False)
            b.interaction['neg_item_id'] = neg
        if gs is not None:
            gs.step(b)
            return
        opt.zero_grad()
        loss = model.calculate_loss(b)
        loss.backward()
        opt.step()

    if ce:
        return _c3_ce_record(dev, step, opt, model, batches, loss, steps, warmup, n_items, B, L,
                             d)
    t = _timed(step, steps, warmup, opt)
    from recbole_amd.model.sequential_recommender.sasrec import _SampledSoftmaxFn
    b0 = batches[0]
    S = torch.randn(B, d, device=dev)
    W = model.item_embedding.weight
    neg = ops.sample_walk(random_list, pr, b0['user_id'], n_neg, None, None, 1_000_000, False)
    tk = _event_time(lambda: _SampledSoftmaxFn.apply(S, W, b0['item_id'], neg))
    k9_bytes = B * (1 + n_neg) * (d * 4 + 8 + d * 4) + B * d * 4 * 2
    # the timed step's dominant kernel (profiles/r03_C3_step.json): the attention backward
    # of torch's fused scaled_dot_product_attention (a library kernel, 2 launches per step:
    # one per layer), timed live with HIP events at the step's shapes (B x heads x L x
    # d/heads, the model's additive mask, its attention dropout). FLOPs per launch: the
    # flash backward's five L x L x dh matmuls (S recomputed, dV, dP, dQ, dK).
    H = config['n_heads']
    dh = d // H
    seq0 = b0['item_id_list']
    mask = model.get_attention_mask(seq0)
    mha = model.trm_encoder.layer[0].multi_head_attention
    p_drop = mha.attn_dropout.p
    from recbole_amd.model import layers as _layers
    k9e = _layers.attn_k9e_applies(torch.empty(B, L, d, device=dev), mask, H, dh)
    if k9e:   # K9e (csrc/attn.hip), the step's own attention: forward, then backward
        q, k, v = (torch.randn(B, L, d, device=dev, requires_grad=True) for _ in range(3))
        rng = mha._k9e_rng(q.device) if p_drop > 0 else None
        o = _layers._AttnFn.apply(q, k, v, mask, H, p_drop, rng)
        ta_fwd = _event_time(lambda: _layers._AttnFn.apply(q.detach(), k.detach(), v.detach(),
                                                           mask, H, p_drop, rng))
    else:
        q, k, v = (torch.randn(B, H, L, dh, device=dev, requires_grad=True) for _ in range(3))
        o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask,
                                                             dropout_p=p_drop)
        ta_fwd = None
    go = torch.randn_like(o)
    ta = _event_time(lambda: torch.autograd.grad(o, (q, k, v), go, retain_graph=True))
    attn_flops = 5 * 2 * B * H * L * L * dh
    flops = 86.3e6 * B    # transformer fwd+bwd per sequence
    cpu = None
    if CPU_BASELINE:
        from oracle import cpu_baseline as cb
        thr, how = cb.host_threads()
        runs = [cb.time_sasrec_steps(batches, random_list.cpu().numpy(), n_items, L, d, n_neg,
                                     steps=8, warmup=1, threads=thr) for _ in range(3)]
        sps, used = float(np.median([r[0] for r in runs])), runs[0][2]
        vals = np.array([r[0] for r in runs])
        cpu = {'value': round(sps, 1), 'unit': 'sequences/s', 'cores': used, 'kind': 'port',
               'threads_derivation': how, 'runs': [round(r[0], 1) for r in runs],
               'cv': round(float(vals.std() / vals.mean()), 4),
               'sample': f'median of 3 runs of 1 warm-up + 8 timed C3 steps of the oracle '
                         f'restatement on torch CPU (numpy walk, SASRecCPU + sampled softmax, '
                         f'dense optim.Adam over the 1.5 GB item table), '
                         f'{sum(r[1] for r in runs):.1f} s timed in all; bounded below the '
                         f'20 + 200 of SURVEY.md 8d (~3 s per CPU step), the run-to-run spread '
                         f'(cv) is reported'}
    return {
        'cpu_baseline': cpu,
        'adam_mode': ADAM_MODE,
        'config': 'C3', 'metric': 'train sequences/s', 'value': round(B / t, 1),
        'unit': 'sequences/s', 'ms_per_step': round(t * 1e3, 3), 'batch': B, 'steps': steps,
        'workload': f'SASRec Amazon-Books-shape: {n_items:,} items (incl. PAD), L={L}, d={d}, '
                    f'2 layers x 2 heads, inner 256, sampled softmax over {n_neg} walk '
                    f'negatives, dense Adam',
        'dtype': 'fp32', 'data': 'synthetic (Zipf(1.1) items, Poisson(20)+4 lengths, seeded)',
        'transformer_tflops_at_step_rate': round(flops / t / 1e12, 2),
        'step_breakdown': _step_breakdown('C3'),
        'roofline': {'kernel': ('K9e attn_bwd_kernel (csrc/attn.hip: the attention backward, '
                                'one workgroup per sequence x head; P recomputed, dP, dS, dQ, '
                                'dK, dV on fp32 MFMA)') if k9e else
                               ('attention backward of torch scaled_dot_product_attention '
                                '(bwd_kernel_fuse, library)'),
                     'bound': 'mfma', 'achieved': round(attn_flops / ta / 1e12, 2),
                     'peak': 157.3, 'unit': 'TFLOP/s',
                     'frac': round(attn_flops / ta / 1e12 / 157.3, 4),
                     'flops_per_launch': attn_flops, 'launch_us': round(ta * 1e6, 1),
                     'fwd_us': round(ta_fwd * 1e6, 1) if ta_fwd else None,
                     'fwd_tflops': (round(2 * 2 * B * H * L * L * dh / ta_fwd / 1e12, 2)
                                    if ta_fwd else None),
                     'timing': 'HIP events around the backward (torch.autograd.grad) of one '
                               'attention at the step shapes, and around one forward (median '
                               'of 10, host-inclusive)',
                     'note': 'fp32 dense MFMA peak; FLOPs of the five L x L x dh products of '
                             'the backward (S recomputed, dV, dP, dQ, dK)'},
        'k9b': _k9b_line(d, n_neg, k9_bytes, tk),
    }


def bench_c3_gru4rec(dev, steps, warmup, scale=1.0, B=2048, L=50, E=64, H=128, n_batches=8,
                     loss='SSM'):
    """The C3-shaped step (bench_c3's batches: Zipf(1.1) items, Poisson(20)+4 lengths, the
    3,000,000-row item table) through GRU4Rec: BPR with one walk negative per sequence
    (loss 'SSM': GRU4Rec has no sampled softmax) or the full-catalogue cross entropy."""
    if loss not in C3_LOSSES:
        raise ValueError(f'loss must be one of {C3_LOSSES}')
    ce = loss != 'SSM'
    from recbole_amd import ops
    from recbole_amd.config import Config
    from recbole_amd.data.interaction import Interaction
    from recbole_amd.model.sequential_recommender import GRU4Rec
    from recbole_amd.trainer.optim import FusedAdam
    from recbole_amd.utils import FeatureType
    n_items = max(1000, int(3_000_000 * scale)) + 1
    config = Config(model='GRU4Rec', dataset='books-synth', config_dict={
        'embedding_size': E, 'hidden_size': H, 'MAX_ITEM_LIST_LENGTH': L,
        'loss_type': 'CE' if ce else 'BPR', 'training_neg_sample_num': 0 if ce else 1,
        'ce_kernel': {'CE-library': 'library', 'CE-fused': 'fused'}.get(loss),
        'state': 'ERROR', 'data_path': ROOT})
    config['device'] = dev
    torch.manual_seed(2020)
    model = GRU4Rec(config, StubDataset({'item_id': FeatureType.TOKEN},
                                        {'item_id': n_items})).to(dev)
    rng = np.random.default_rng(2020)
    batches = []
    for _ in range(n_batches):
        lens = np.minimum(rng.poisson(20, B) + 4, L).astype(np.int64)
        seq = np.zeros((B, L), dtype=np.int64)
        ids = _zipf_ids(rng, 1.1, int(lens.sum()), n_items - 1)
        mask = np.arange(L)[None, :] < lens[:, None]
        seq[mask] = ids
        batches.append(Interaction({
            'item_id_list': torch.as_tensor(seq), 'item_length': torch.as_tensor(lens),
            'item_id': torch.as_tensor(_zipf_ids(rng, 1.1, B, n_items - 1)),
            'user_id': torch.as_tensor(rng.integers(1, 1_000_000, B))}).to(dev))
    random_list = torch.as_tensor(rng.permutation(np.arange(1, n_items)).astype(np.int32),
                                  device=dev)
    pr = torch.zeros(1, dtype=torch.int64, device=dev)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    if ADAM_MODE == 'deferred':
        opt.enable_deferred(model.deferred_tables())
    it = [0]
    gs = None
    graphed = GRAPH_STEP and model.graph_step_safe      # as the Trainer decides
    if graphed:
        from recbole_amd.trainer.graph_step import GraphedTrainStep
        gs = GraphedTrainStep(model, opt)

    def step():
        b = batches[it[0] % n_batches]
        it[0] += 1
        if not ce:
            b.interaction['neg_item_id'] = ops.sample_walk(random_list, pr, b['user_id'], 1,
                                                           None, None, 1_000_000, False)
        if gs is not None:
            gs.step(b)
            return
        opt.zero_grad()
        loss_ = model.calculate_loss(b)
        loss_.backward()
        opt.step()

    t = _timed(step, steps, warmup, opt)
    return {
        'config': 'C3', 'model': 'GRU4Rec',
        'loss': 'BPR' if not ce else loss, 'metric': 'train sequences/s',
        'value': round(B / t, 1), 'unit': 'sequences/s', 'ms_per_step': round(t * 1e3, 3),
        'batch': B, 'steps': steps, 'adam_mode': ADAM_MODE, 'graph_step': graphed,
        'workload': f'GRU4Rec Amazon-Books-shape: {n_items:,} items (incl. PAD), L={L}, '
                    f'E={E}, H={H}, 1 layer, dropout 0.3, dense Adam',
        'dtype': 'fp32', 'data': 'synthetic (Zipf(1.1) items, Poisson(20)+4 lengths, seeded)',
        'peak_allocated_MB': round(torch.cuda.max_memory_allocated(dev) / 1e6, 1),
    }


def bench_neumf(dev, steps, warmup, scale=1.0, B=2048, K=10, generic_users=256):
    """NeuMF at C2's table shape (138,494 users x 26,745 items incl. the pad rows, default
    widths 64 / 64 / [128, 64, 32]): the pointwise train step (B positives + B walk-free
    uniform negatives with labels, samples/s), the fused full-sort evaluation of every user
    (K14c, users/s, with the kernel's share of the fp32 MFMA peak at
    2 * sum H_l H_{l+1} + 2 * dmf flops per pair for layers 2..L) and the generic fallback
    (fused_eval: False — one user per batch repeated over the catalogue, predict in
    eval_batch_size pieces, mask, topk) on `generic_users` users."""
    from recbole_amd import ops
    from recbole_amd.config import Config
    from recbole_amd.data.interaction import Interaction
    from recbole_amd.model.general_recommender import NeuMF
    from recbole_amd.trainer.optim import FusedAdam
    from recbole_amd.utils import FeatureType
    nU, nI = max(2000, int(138_493 * scale)) + 1, max(1000, int(26_744 * scale)) + 1
    config = Config(model='NeuMF', dataset='ml20m-synth', config_dict={
        'state': 'ERROR', 'data_path': ROOT, 'load_col': None})
    config['device'] = dev
    torch.manual_seed(2020)
    model = NeuMF(config, StubDataset({'user_id': FeatureType.TOKEN, 'item_id': FeatureType.TOKEN},
                                      {'user_id': nU, 'item_id': nI})).to(dev)
    rng = np.random.default_rng(2020)
    batches = []
    for _ in range(8):
        batches.append(Interaction({
            'user_id': torch.as_tensor(np.tile(rng.integers(1, nU, B), 2)),
            'item_id': torch.as_tensor(np.r_[_zipf_ids(rng, 1.1, B, nI - 1), rng.integers(1, nI, B)]),
            'label': torch.as_tensor(np.r_[np.ones(B), np.zeros(B)].astype(np.float32))}).to(dev))
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=config['weight_decay'])
    if ADAM_MODE == 'deferred':
        opt.enable_deferred(model.deferred_tables())
    it = [0]

    def step():
        b = batches[it[0] % len(batches)]
        it[0] += 1
        opt.zero_grad()
        model.calculate_loss(b).backward()
        opt.step()

    t_train = _timed(step, steps, warmup, opt)
    opt.flush()
    model.eval()
    # evaluation inputs: ~20 history items and 1..3 positives per user, sorted CSRs
    def sorted_rows(width, counts):
        """Per row up to counts[r] distinct sorted ids of 1..nI-1 as a CSR."""
        a = np.sort(rng.integers(1, nI, (nU - 1, width)), axis=1)
        keep = np.ones(a.shape, dtype=bool)
        keep[:, 1:] = a[:, 1:] != a[:, :-1]
        keep &= np.cumsum(keep, axis=1) <= counts[:, None]
        return np.r_[0, np.cumsum(keep.sum(1))].astype(np.int64), a[keep].astype(np.int32)

    hist_ptr, hist_cols = sorted_rows(30, rng.integers(10, 31, nU - 1))
    pos_ptr, pos_cols = sorted_rows(3, rng.integers(1, 4, nU - 1))
    D = lambda a: torch.as_tensor(a, device=dev)
    uids = torch.arange(1, nU, device=dev)
    hp, hc, pp, pc = D(hist_ptr), D(hist_cols), D(pos_ptr), D(pos_cols)
    n = uids.numel()

    def fused():
        scorer = model.fused_pair_scorer()
        return scorer.topk(uids, K, hist_ptr=hp, hist_cols=hc, pos_ptr=pp, pos_cols=pc)

    with torch.no_grad():
        fused()
        torch.cuda.synchronize()
        t_fused = _event_time(fused, reps=3)
        ops.KERNEL_EVENTS = {'pair_mlp': []}
        try:
            flags = fused()['pos_flags']
            torch.cuda.synchronize()
            t_kernel = float(np.mean([a.elapsed_time(b) * 1e-3 for a, b in ops.KERNEL_EVENTS['pair_mlp']]))
        finally:
            ops.KERNEL_EVENTS = None
        test_bs = config['eval_batch_size']
        items = torch.arange(nI, device=dev)
        g_n = min(generic_users, n)

        def generic():
            out = []
            for q in range(g_n):                     # FULL loader: eval_batch_size // n_items users
                users = uids[q:q + 1].repeat_interleave(nI)
                scores = torch.cat([model.predict({'user_id': users[i:i + test_bs],
                                                   'item_id': items[i:i + test_bs]})
                                    for i in range(0, nI, test_bs)])
                scores[0] = -np.inf
                scores[hc[hist_ptr[q]:hist_ptr[q + 1]].long()] = -np.inf
                out.append(torch.topk(scores, K).indices)
            return torch.stack(out)

        generic()
        torch.cuda.synchronize()
        t_generic = _event_time(generic, reps=2)
        g_ids = generic().cpu().numpy()
        f_ids = fused()['ids'][:g_n].cpu().numpy()
    hs = list(model.mlp_hidden_size)
    flops_pair = 2 * sum(a * b for a, b in zip(hs[:-1], hs[1:])) + 2 * model.mf_embedding_size
    tf = flops_pair * n * nI / t_kernel / 1e12
    return {
        'config': 'N2', 'model': 'NeuMF', 'metric': 'train samples/s',
        'value': round(2 * B / t_train, 1), 'unit': 'samples/s',
        'ms_per_step': round(t_train * 1e3, 3), 'batch': 2 * B, 'steps': steps,
        'adam_mode': ADAM_MODE, 'graph_step': False,
        'eval_fused': {'metric': 'full-sort eval users/s', 'value': round(n / t_fused, 1),
                       'users': n, 'items': nI, 'seconds': round(t_fused, 4),
                       'k14c_seconds': round(t_kernel, 4), 'flops_per_pair': flops_pair,
                       'k14c_tflops': round(tf, 2),
                       'k14c_frac_of_fp32_mfma_peak': round(tf / MFMA_F32_PEAK_TFLOPS, 3),
                       'hit_rows': int(flags.any(dim=1).sum().item())},
        'eval_generic': {'metric': 'full-sort eval users/s (fused_eval: False sequence)',
                         'value': round(g_n / t_generic, 1), 'users': g_n,
                         'seconds': round(t_generic, 4),
                         'ids_equal_to_fused': float((g_ids == f_ids).mean())},
        'eval_speedup': round((n / t_fused) / (g_n / t_generic), 1),
        'workload': f'NeuMF ML-20M-shape: {nU:,} users x {nI:,} items (incl. pad rows), '
                    f'mf 64, mlp 64, hidden {hs}, BCE, weight_decay 1e-8, top-{K}',
        'dtype': 'fp32', 'data': 'synthetic (uniform users, Zipf(1.1) positives, seeded)',
        'peak_allocated_MB': round(torch.cuda.max_memory_allocated(dev) / 1e6, 1),
    }


def bench_multivae(dev, steps, warmup, scale=1.0, B=2048, K=10, generic_users=256):
    """MultiVAE at C2's table shape (138,494 users x 26,745 items incl. the pad rows, the
    synthetic ml-20m-shape interactions of bench.make_c2 as every user's history), default
    widths (600, latent 128, dropout 0.5), B users per step.

    train: the K15 step (K15a -> layers -> addmm -> K15c, backward K15c in place / K15b)
      against a DENSE statement of the reference's step written here with torch ops: the
      [B, n_items] rating matrix by index_put_, F.normalize, F.dropout, the encoder's first
      layer as a dense GEMM, log_softmax(z) * rating_matrix. Same device, same initial
      weights, same user batches, FusedAdam for both; peak allocated bytes of each.
    eval: every user's full-sort top-K, fused (score blocks of MATRIX_EVAL_BYTES + K15d)
      against the generic sequence (full_sort_predict, the pad / history mask, torch.topk;
      one user per batch, as eval_batch_size 4,096 gives at this catalogue) on
      `generic_users` users."""
    import copy

    import torch.nn.functional as F

    import bench
    from recbole_amd import ops
    from recbole_amd.config import Config
    from recbole_amd.data.dataset import Dataset
    from recbole_amd.model.general_recommender import MultiVAE
    from recbole_amd.trainer.fused_eval import MATRIX_EVAL_BYTES
    from recbole_amd.trainer.optim import FusedAdam
    n_u, n_i = max(2000, int(138_493 * scale)), max(1000, int(26_744 * scale))
    u, i, nU, nI = bench.make_c2(2020, n_u, n_i, int(20_000_263 * scale))
    config = Config(model='MultiVAE', dataset='ml20m-synth', config_dict={
        'state': 'ERROR', 'data_path': ROOT, 'load_col': None})
    config['device'] = dev
    torch.manual_seed(2020)
    model = MultiVAE(config, Dataset.from_interactions(config, u, i, nU, nI)).to(dev)
    dense = copy.deepcopy(model)
    nnz_row = model.hist_cols.numel() / (nU - 1)
    rng = np.random.default_rng(2020)
    batches = [torch.as_tensor(rng.integers(0, nU, B)).to(dev) for _ in range(8)]

    def runner(m, loss_fn):
        opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=config['weight_decay'])
        it = [0]

        def step():
            b = batches[it[0] % len(batches)]
            it[0] += 1
            opt.zero_grad()
            loss_fn(m, b).backward()
            opt.step()
        return step, opt

    def dense_loss(m, user):
        m.update += 1
        anneal = min(m.anneal_cap, m.update / m.total_anneal_steps)
        R = m.get_rating_matrix(user)
        h = m.encoder(F.dropout(F.normalize(R), m.drop_out, training=True))
        half = m.lat_dim // 2
        mu, logvar = h[:, :half], h[:, half:]
        z = m.decoder(mu + torch.zeros_like(logvar).normal_(0, 0.01) * torch.exp(0.5 * logvar))
        kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1)) * anneal
        return -(F.log_softmax(z, 1) * R).sum(1).mean() + kl

    out = {}
    for name, m, fn in (('k15', model, lambda m, b: m.calculate_loss({'user_id': b})),
                        ('dense', dense, dense_loss)):
        m.train()
        step, opt = runner(m, fn)
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t = _timed(step, steps, warmup, opt)
        out[name] = {'ms_per_step': round(t * 1e3, 3), 'users_per_s': round(B / t, 1),
                     'peak_allocated_MB': round(torch.cuda.max_memory_allocated(dev) / 1e6, 1)}
        del step, opt
    del dense
    torch.cuda.empty_cache()

    model.eval()
    uids = torch.arange(1, nU, device=dev)
    n = uids.numel()
    hp, hc = model.hist_ptr[1:].contiguous(), model.hist_cols      # users 1.. of the CSR
    pos = np.sort(rng.integers(1, nI, (n, 2)), axis=1)
    pp = torch.arange(0, 2 * n + 1, 2, device=dev)
    pc = torch.as_tensor(pos.reshape(-1).astype(np.int32), device=dev)
    block = max(1, MATRIX_EVAL_BYTES // (4 * nI))
    g_n = min(generic_users, n)

    def fused(count=n):
        scorer = model.fused_matrix_scorer()
        flags = torch.empty(count, K, dtype=torch.uint8, device=dev)
        ids = torch.empty(count, K, dtype=torch.int32, device=dev)
        for s0 in range(0, count, block):
            e0 = min(count, s0 + block)
            ops.matrix_topk(scorer.scores(uids[s0:e0]), K, hist_ptr=hp[s0:e0 + 1], hist_cols=hc,
                            pos_ptr=pp[s0:e0 + 1], pos_cols=pc,
                            out={'pos_flags': flags[s0:e0], 'ids': ids[s0:e0]})
        return flags, ids

    def generic():
        res = []
        for q in range(g_n):
            scores = model.full_sort_predict({'user_id': uids[q:q + 1]}).view(1, nI)
            scores[:, 0] = -np.inf
            scores[0, hc[hp[q]:hp[q + 1]].long()] = -np.inf
            res.append(torch.topk(scores, K).indices)
        return torch.cat(res)

    with torch.no_grad():
        fused()
        torch.cuda.synchronize()
        t_fused = _event_time(fused, reps=3)
        generic()
        torch.cuda.synchronize()
        t_generic = _event_time(generic, reps=2)
        same = float((generic().cpu().numpy() == fused(g_n)[1].cpu().numpy()).mean())
    return {
        'config': 'A2', 'model': 'MultiVAE', 'metric': 'train users/s',
        'value': out['k15']['users_per_s'], 'unit': 'users/s', 'batch': B, 'steps': steps,
        'train_k15': out['k15'], 'train_dense_torch': out['dense'],
        'train_speedup': round(out['dense']['ms_per_step'] / out['k15']['ms_per_step'], 2),
        'eval_fused': {'metric': 'full-sort eval users/s', 'value': round(n / t_fused, 1),
                       'users': n, 'seconds': round(t_fused, 4), 'users_per_block': block},
        'eval_generic': {'metric': 'full-sort eval users/s (fused_eval: False sequence)',
                         'value': round(g_n / t_generic, 1), 'users': g_n,
                         'seconds': round(t_generic, 4), 'ids_equal_to_fused': same},
        'eval_speedup': round((n / t_fused) / (g_n / t_generic), 1),
        'workload': f'MultiVAE ML-20M-shape: {nU:,} users x {nI:,} items (incl. pad rows), '
                    f'{model.hist_cols.numel():,} interactions ({nnz_row:.1f} per user), hidden '
                    f'{list(model.layers)}, latent {model.lat_dim}, dropout {model.drop_out}, '
                    f'top-{K}',
        'dtype': 'fp32', 'graph_step': False,
        'data': 'synthetic (bench.make_c2: lognormal user activity, Zipf items, seeded)',
        'sample': 'one run; spread not measured',
    }


def _reference_cloze_loop(item_seq, mask_ratio, M, n_items, mask_token):
    """BERT4Rec.reconstruct_train_data as the reference runs it (bert4rec.py:111-156): the
    batch copied to the host, Python lists, random.random() per position, a rejection-sampled
    negative per masked item, four tensors built on the device. Returns them."""
    import random

    def pad(sequence, max_length):
        sequence = [0] * (max_length - len(sequence)) + sequence
        return sequence[-max_length:]
    device = item_seq.device
    batch_size = item_seq.size(0)
    instances = item_seq.cpu().numpy().tolist()
    seqs, poss, negs, idxs = [], [], [], []
    for instance in instances:
        masked_sequence = instance.copy()
        pos_item, neg_item, index_ids = [], [], []
        for index_id, item in enumerate(instance):
            if item == 0:
                break
            if random.random() < mask_ratio:
                pos_item.append(item)
                neg = random.randint(1, n_items - 1)
                while neg in instance:
                    neg = random.randint(1, n_items - 1)
                neg_item.append(neg)
                masked_sequence[index_id] = mask_token
                index_ids.append(index_id)
        seqs.append(masked_sequence)
        poss.append(pad(pos_item, M))
        negs.append(pad(neg_item, M))
        idxs.append(pad(index_ids, M))
    return tuple(torch.tensor(x, dtype=torch.long, device=device).view(batch_size, -1)
                 for x in (seqs, poss, negs, idxs))


def bench_bert4rec(dev, steps, warmup, scale=1.0, B=1024, L=50, d=128, n_batches=8):
    """B3: the BERT4Rec training step, ce_kernel 'fused' against 'library' on the same
    weights and batches (each in its own timed window, peak memory reset between them), and
    the Cloze masking alone: K17a against the reference's host loop."""
    from recbole_amd import ops
    from recbole_amd.config import Config
    from recbole_amd.data.interaction import Interaction
    from recbole_amd.model.sequential_recommender import BERT4Rec
    from recbole_amd.trainer.optim import FusedAdam
    from recbole_amd.utils import FeatureType
    n_items = max(1000, int(65_536 * scale)) + 1
    rng = np.random.default_rng(2020)
    batches = []
    for _ in range(n_batches):
        lens = np.minimum(rng.poisson(20, B) + 4, L).astype(np.int64)
        seq = np.zeros((B, L), dtype=np.int64)
        seq[np.arange(L)[None, :] < lens[:, None]] = _zipf_ids(rng, 1.1, int(lens.sum()),
                                                               n_items - 1)
        batches.append(Interaction({'item_id_list': torch.as_tensor(seq),
                                    'item_length': torch.as_tensor(lens)}).to(dev))
    state, out = None, {}
    for kernel in ('fused', 'library'):
        config = Config(model='BERT4Rec', dataset='b3-synth', config_dict={
            'hidden_size': d, 'n_heads': 2, 'inner_size': 256, 'MAX_ITEM_LIST_LENGTH': L,
            'mask_ratio': 0.2, 'loss_type': 'CE', 'ce_kernel': kernel,
            'training_neg_sample_num': 0, 'state': 'ERROR', 'data_path': ROOT,
            'load_col': None})
        config['device'] = dev
        torch.manual_seed(2020)
        model = BERT4Rec(config, StubDataset({'item_id': FeatureType.TOKEN},
                                             {'item_id': n_items})).to(dev)
        if state is None:
            state = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(state)
        opt = FusedAdam(model.parameters(), lr=1e-3)
        it = [0]

        def step():
            b = batches[it[0] % n_batches]
            it[0] += 1
            opt.zero_grad()
            loss_ = model.calculate_loss(b)
            loss_.backward()
            opt.step()
            return loss_

        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        t = _timed(step, steps, warmup, opt)
        out[kernel] = {'steps_per_s': round(1.0 / t, 2), 'ms_per_step': round(t * 1e3, 3),
                       'sequences_per_s': round(B / t, 1),
                       'peak_allocated_MB': round(torch.cuda.max_memory_allocated(dev) / 1e6, 1),
                       'last_loss': round(float(step().item()), 4)}
        M, ratio = model.mask_item_length, model.mask_ratio
        del model, opt
    seq0 = batches[0]['item_id_list']
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    k17a = _event_time(lambda: ops.cloze_mask(seq0, M, n_items, ratio, 2020, counter, False))
    k17a_neg = _event_time(lambda: ops.cloze_mask(seq0, M, n_items, ratio, 2020, counter, True))
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _reference_cloze_loop(seq0, ratio, M, n_items, n_items)
        torch.cuda.synchronize()
        host.append(time.perf_counter() - t0)
    return {
        'config': 'B3', 'model': 'BERT4Rec', 'metric': 'train steps/s (ce_kernel fused)',
        'value': out['fused']['steps_per_s'], 'unit': 'steps/s', 'batch': B, 'steps': steps,
        'fused': out['fused'], 'library': out['library'],
        'fused_over_library': round(out['library']['ms_per_step'] / out['fused']['ms_per_step'],
                                    3),
        'library_logits_MB': round(B * M * n_items * 4 / 1e6, 1),
        'cloze_mask': {
            'k17a_us': round(k17a * 1e6, 1), 'k17a_with_negatives_us': round(k17a_neg * 1e6, 1),
            'reference_host_loop_ms': round(float(np.median(host)) * 1e3, 2),
            'timing': 'K17a: HIP events around one ops.cloze_mask (the launch and its four '
                      'output allocations), median of 10; host loop: wall time of the '
                      "reference's reconstruct_train_data restated in pure Python on the same "
                      'batch (device -> host copy, loop, four tensors back), median of 3'},
        'workload': f'BERT4Rec: {n_items:,} items (incl. PAD) + mask token, L={L}, d={d}, '
                    f'2 layers, 2 heads, inner 256, dropout 0.5, mask_ratio 0.2 (M={M}), '
                    f'dense Adam, eager step',
        'dtype': 'fp32', 'data': 'synthetic (Zipf(1.1) items, Poisson(20)+4 lengths, seeded)',
    }


def _c3_ce_record(dev, step, opt, model, batches, loss, steps, warmup, n_items, B, L, d):
    """The C3 step with the full-catalogue cross entropy: sequences/s, the peak allocated
    memory of the run (measured before the loss-only timings below), and the loss's own forward / backward call times (HIP
    events, host-inclusive; the per-kernel split of K12a / K12b / K12c comes from a kernel
    trace of this leg, tools/step_breakdown.py). One GEMM pass over the logits is
    2 * B * I * d FLOPs: the library path makes 3 (logits, dS, dE), K12 makes 5 (K12a 1,
    K12b 2, K12c 2: each backward kernel recomputes its logits tile)."""
    from recbole_amd import ops
    t = _timed(step, steps, warmup, opt)
    # over the whole run, the warm-up included: the captured step allocates while it is
    # captured (its replays reuse that pool and allocate nothing)
    peak = torch.cuda.max_memory_allocated(dev)
    reserved = torch.cuda.max_memory_reserved(dev)
    gemm = 2 * B * n_items * d
    S = torch.randn(B, d, device=dev) * 0.05
    W = model.item_embedding.weight.detach()
    tgt = batches[0]['item_id']
    rec = {
        'config': 'C3', 'loss': loss, 'metric': 'train sequences/s', 'value': round(B / t, 1),
        'unit': 'sequences/s', 'ms_per_step': round(t * 1e3, 3), 'batch': B, 'steps': steps,
        'adam_mode': ADAM_MODE, 'graph_step': GRAPH_STEP,
        'workload': f'SASRec Amazon-Books-shape: {n_items:,} items (incl. PAD), L={L}, d={d}, '
                    f'2 layers x 2 heads, inner 256, full-catalogue cross entropy ({loss}), '
                    f'dense Adam',
        'dtype': 'fp32',
        'peak_allocated_MB': round(peak / 1e6, 1),
        'peak_reserved_MB': round(reserved / 1e6, 1),
        'logits_matrix_MB': round(B * n_items * 4 / 1e6, 1),
        'gemm_pass_gflop': round(gemm / 1e9, 2),
    }
    if loss == 'CE-fused':
        g1 = torch.ones(1, device=dev)
        lse, _ = ops.full_ce_fwd(S, W, tgt)
        tf = _event_time(lambda: ops.full_ce_fwd(S, W, tgt))
        tb = _event_time(lambda: ops.full_ce_bwd(S, W, tgt, lse, g1))
        rec['k12'] = {
            'splits': ops.full_ce_splits(B, n_items, d, 0),
            'fwd_call_us': round(tf * 1e6, 1), 'bwd_call_us': round(tb * 1e6, 1),
            'fwd_tflops': round(gemm / tf / 1e12, 2), 'bwd_tflops': round(4 * gemm / tb / 1e12, 2),
            'fwd_frac_of_peak': round(gemm / tf / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
            'bwd_frac_of_peak': round(4 * gemm / tb / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
            'timing': 'HIP events around one ops.full_ce_fwd (K12a + finish) and one '
                      'ops.full_ce_bwd (K12b + partial sum + K12c), median of 10, '
                      'host-inclusive; FLOPs 1 and 4 GEMM passes of 2*B*I*d'}
    else:
        Sg = S.clone().requires_grad_()
        Wg = W.clone().requires_grad_()

        def lib_ce():
            l_ = torch.nn.functional.cross_entropy(torch.matmul(Sg, Wg.transpose(0, 1)), tgt)
            torch.autograd.grad(l_, (Sg, Wg))
        lib_ce()
        tl = _event_time(lib_ce)
        rec['library_ce'] = {
            'fwd_bwd_call_us': round(tl * 1e6, 1),
            'tflops': round(3 * gemm / tl / 1e12, 2),
            'timing': 'HIP events around matmul + cross_entropy + autograd.grad, median of '
                      '10, host-inclusive; FLOPs 3 GEMM passes of 2*B*I*d'}
    return rec


def _k9b_line(d, n_neg, k9_bytes, tk):
    """K9b's roofline on its kernel time in the committed C3 step trace (rocprofv3,
    profiles/r*_C3_step.json: the launch inside the captured step), the host-inclusive
    HIP-event time of an eager launch beside it."""
    import glob
    import json
    t_trace, src = None, None
    for path in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_C3_step.json')))[::-1]:
        ks = [k for k in json.load(open(path))['kernels'] if 'sampled_softmax' in k['kernel']]
        if ks:
            t_trace, src = ks[0]['avg_us'] * 1e-6, os.path.basename(path)
            break
    t = t_trace if t_trace is not None else tk
    return {'kernel': f'K9b sampled_softmax<{d}> ({n_neg} negatives)', 'bound': 'hbm',
            'achieved': round(k9_bytes / t / 1e9, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
            'frac': round(k9_bytes / t / 1e9 / HBM_PEAK_GBS, 4), 'bytes_per_launch': k9_bytes,
            'launch_us': round(t * 1e6, 1), 'timing_source': src or 'HIP events (eager)',
            'launch_us_incl_host': round(tk * 1e6, 1)}


# ----------------------------------------------------------------------------- C5
def make_c5_graph(n_users, n_items, nnz, seed=2020):
    """Distinct (user, item) edges: user degrees Zipf-like (min 1), items Zipf(1.0)."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, n_users + 1) ** 0.6
    deg = np.maximum(1, np.round(w / w.sum() * nnz)).astype(np.int64)
    deg = np.minimum(deg, n_items // 2)
    u = np.repeat(rng.permutation(np.arange(1, n_users + 1)), deg[rng.permutation(n_users)])
    p = 1.0 / np.arange(1, n_items + 1)
    cdf = np.cumsum(p / p.sum())
    i = np.searchsorted(cdf, rng.random(len(u))).astype(np.int64) + 1
    i = np.minimum(i, n_items)
    key = np.unique(u * (n_items + 1) + i)
    return key // (n_items + 1), key % (n_items + 1)


def bench_c5(dev, scale=1.0, d=256, n_layers=2, K=10, sample_users=131072):
    from recbole_amd import ops
    from recbole_amd.model.general_recommender.lightgcn import norm_adj_csr, propagate
    U = int(10_000_000 * scale) + 1
    I = int(5_000_000 * scale) + 1
    t0 = time.perf_counter()
    u, i = make_c5_graph(U - 1, I - 1, int(100_000_000 * scale))
    print(f'C5: {len(u):,} edges generated ({time.perf_counter() - t0:.0f} s)', file=sys.stderr,
          flush=True)
    rp, cols, vals = norm_adj_csr(u, i, U, I)
    print(f'C5: normalised adjacency built ({time.perf_counter() - t0:.0f} s)', file=sys.stderr,
          flush=True)
    plan = ops.SpmmPlan(rp, cols, vals, device=dev)
    setup = time.perf_counter() - t0
    g = torch.Generator(device=dev).manual_seed(2020)
    EU = torch.randn(U, d, generator=g, device=dev) * 0.01
    EI = torch.randn(I, d, generator=g, device=dev) * 0.01
    out_u, out_i = torch.empty_like(EU), torch.empty_like(EI)
    tmp = [torch.empty(U + I, d, device=dev)]
    propagate(plan, EU, EI, n_layers, out_u, out_i, tmp)      # warm-up
    torch.cuda.synchronize()
    tp = _event_time(lambda: propagate(plan, EU, EI, n_layers, out_u, out_i, tmp), reps=3)
    # K7 algorithmic bytes per layer: per nonzero col+val (8 B) + the gathered row
    # (d*4 B); per row the output write (d*4) and the accumulator read/write
    nnz2 = int(rp[-1])
    per_layer = nnz2 * (8 + d * 4) + (U + I) * (d * 4 * 3) + (U + I + 1) * 8
    # full-sort sample: users 1..n, history = their training edges, 1 positive each
    n = min(sample_users, U - 1)
    users = torch.arange(1, n + 1, device=dev)
    up = rp[:U + 1]
    hist_ptr = torch.as_tensor((up[1:n + 2] - up[1]).astype(np.int64), device=dev)
    hist_cols = torch.as_tensor((cols[up[1]:up[n + 1]].astype(np.int64) - U).astype(np.int32),
                                device=dev)
    rng = np.random.default_rng(7)
    pos_cols = torch.as_tensor(rng.integers(1, I, n).astype(np.int32), device=dev)
    pos_ptr = torch.arange(n + 1, dtype=torch.int64, device=dev)
    Uq = ops.gather_rows(out_u, users)
    o = {}
    run = lambda: ops.fullsort_topk(Uq, out_i, K, hist_ptr=hist_ptr, hist_cols=hist_cols,
                                    pos_ptr=pos_ptr, pos_cols=pos_cols, out=o)
    run()
    torch.cuda.synchronize()
    tf = _event_time(run, reps=3)
    flops = 2.0 * n * I * d
    cpu = None
    if CPU_BASELINE:
        from oracle import cpu_baseline as cb
        thr, how = cb.host_threads()
        nc = 512
        uq, it = Uq[:nc].cpu(), out_i.cpu()
        runs = [cb.time_full_sort_users(uq, it, nc, K=K, threads=thr) for _ in range(3)]
        ups, used = float(np.median([r[0] for r in runs])), runs[0][2]
        cpu = {'value': round(ups, 1), 'unit': 'users/s', 'cores': used, 'kind': 'port',
               'threads_derivation': how, 'runs': [round(r[0], 1) for r in runs],
               'sample': f'median of 3 runs of {nc} users ranked on torch CPU as the reference '
                         f'does (U[u] @ I^T, pad mask, flip + topk), '
                         f'{sum(r[1] for r in runs):.1f} s timed in all'}
    return {
        'cpu_baseline': cpu,
        'config': 'C5', 'metric': 'full-sort eval users/s', 'value': round(n / tf, 1),
        'unit': 'users/s', 'users_timed': n,
        'workload': f'LightGCN {U - 1:,} users x {I - 1:,} items, {len(u):,} edges, d={d}, '
                    f'{n_layers} layers; full-sort top-{K} vs all items with history mask',
        'dtype': 'fp32', 'data': 'synthetic (Zipf items, Zipf-like user degrees, seeded)',
        'setup_s': round(setup, 1),
        'roofline': {'kernel': f'K6 fullsort_topk<{d}> (fp32 MFMA 32x32x2)', 'bound': 'mfma',
                     'achieved': round(flops / tf / 1e12, 2), 'peak': FP32_PEAK_TFLOPS,
                     'unit': 'TFLOP/s', 'frac': round(flops / tf / 1e12 / FP32_PEAK_TFLOPS, 4),
                     'flops_per_launch': flops, 'launch_ms': round(tf * 1e3, 2)},
        'propagation': {'kernel': f'K7 spmm_units_kernel<{d}> x {n_layers} layers',
                        'bound': 'hbm', 'ms': round(tp * 1e3, 2),
                        'achieved': round(n_layers * per_layer / tp / 1e9, 1),
                        'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                        'frac': round(n_layers * per_layer / tp / 1e9 / HBM_PEAK_GBS, 4),
                        'bytes_per_layer': per_layer, 'nnz': nnz2},
        'full_pass_s_estimate': round((U - 1) / (n / tf) + tp, 1),
    }


# ----------------------------------------------------------------------------- G2
def bench_ngcf(dev, steps, warmup, scale=1.0, B=2048, windows=3):
    """One NGCF training step (zero_grad, calculate_loss, backward, FusedAdam) on
    make_c5_graph at `scale`, widths 64 / [64, 64, 64], message dropout 0.1: the model's
    kernel path against the torch op sequence written below, on copies of the same initial
    weights and the same batches. `windows` timed windows of `steps` steps each, the two
    sides alternating; peak allocated memory of each side's windows. Before the timing the
    two steps' loss and gradients are compared on the first batch with the dropout off (the
    two sides draw their masks from different generators)."""
    import copy
    import scipy.sparse as sp
    import torch.nn.functional as F
    from recbole_amd.config import Config
    from recbole_amd.data.interaction import Interaction
    from recbole_amd.model.general_recommender import NGCF
    from recbole_amd.trainer.optim import FusedAdam
    from recbole_amd.utils import FeatureType
    U, I = int(10_000_000 * scale) + 1, int(5_000_000 * scale) + 1
    t0 = time.perf_counter()
    u, i = make_c5_graph(U - 1, I - 1, int(100_000_000 * scale))

    class _Graph(StubDataset):
        def inter_matrix(self, form='coo'):
            return sp.coo_matrix((np.ones(len(u), dtype=np.float32), (u, i)), shape=(U, I))

    config = Config(model='NGCF', dataset='c5-synth', config_dict={
        'state': 'ERROR', 'data_path': ROOT, 'load_col': None})
    config['device'] = dev
    torch.manual_seed(2020)
    model = NGCF(config, _Graph({'user_id': FeatureType.TOKEN, 'item_id': FeatureType.TOKEN},
                                {'user_id': U, 'item_id': I})).to(dev)
    assert model._kernel_path() and list(model.hidden_size_list) == [64, 64, 64, 64]
    twin = copy.deepcopy(model)                       # the torch statement's weights
    A = model._torch_matrix(None, dev).coalesce()
    model.norm_adj_plan                               # the K7 plan, outside the timing
    setup = time.perf_counter() - t0
    rng = np.random.default_rng(2020)
    batches = []
    for _ in range(8):
        e = rng.integers(0, len(u), B)
        batches.append(Interaction({'user_id': torch.as_tensor(u[e]),
                                    'item_id': torch.as_tensor(i[e]),
                                    'neg_item_id': torch.as_tensor(rng.integers(1, I, B))}).to(dev))

    def torch_loss(m, b, p):
        E = torch.cat([m.user_embedding.weight, m.item_embedding.weight], dim=0)
        out = [E]
        for g in m.GNNlayers:
            x = torch.sparse.mm(A, E)
            z = g.linear(E + x) + g.interActTransform(x * E)
            E = F.normalize(F.dropout(F.leaky_relu(z, 0.2), p, True), p=2, dim=1)
            out.append(E)
        ua, ia = torch.split(torch.cat(out, dim=1), [U, I])
        a, ps, ng = ua[b['user_id']], ia[b['item_id']], ia[b['neg_item_id']]
        mf = -torch.log(1e-10 + torch.sigmoid((a * ps).sum(1) - (a * ng).sum(1))).mean()
        return mf + m.reg_weight * (a.norm() + ps.norm() + ng.norm()) / a.shape[0]

    # the two steps' outputs on the first timed batch, dropout off
    model.message_dropout = 0.0
    lk = model.calculate_loss(batches[0])
    lk.backward()
    lt = torch_loss(twin, batches[0], 0.0)
    lt.backward()
    check = {'loss_kernels': lk.item(), 'loss_torch': lt.item(),
             'loss_rel_diff': abs(lk.item() - lt.item()) / abs(lt.item()), 'grad_max_abs_diff': {},
             'grad_max_abs_torch': {}}
    for (name, a), (_, b) in zip(model.named_parameters(), twin.named_parameters()):
        check['grad_max_abs_diff'][name] = float((a.grad - b.grad).abs().max())
        check['grad_max_abs_torch'][name] = float(b.grad.abs().max())
    model.zero_grad(set_to_none=True)
    twin.zero_grad(set_to_none=True)
    model.message_dropout = 0.1

    opt_k = FusedAdam(model.parameters(), lr=1e-3)
    opt_t = FusedAdam(twin.parameters(), lr=1e-3)
    it = [0, 0]

    def step_k():
        b = batches[it[0] % len(batches)]
        it[0] += 1
        opt_k.zero_grad()
        model.calculate_loss(b).backward()
        opt_k.step()

    def step_t():
        b = batches[it[1] % len(batches)]
        it[1] += 1
        opt_t.zero_grad()
        torch_loss(twin, b, 0.1).backward()
        opt_t.step()

    tk, tt, peak = [], [], [0, 0]
    for w in range(windows):
        for side, (fn, ts) in enumerate(((step_k, tk), (step_t, tt))):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            ts.append(_timed(fn, steps, warmup if w == 0 else 1))
            peak[side] = max(peak[side], torch.cuda.max_memory_allocated(dev))
    mk, mt = float(np.median(tk)), float(np.median(tt))
    return {
        'config': 'G2', 'model': 'NGCF', 'metric': 'train steps/s', 'value': round(1 / mk, 2),
        'unit': 'steps/s', 'ms_per_step': round(mk * 1e3, 3),
        'ms_per_step_windows': [round(t * 1e3, 3) for t in tk],
        'torch': {'ms_per_step': round(mt * 1e3, 3),
                  'ms_per_step_windows': [round(t * 1e3, 3) for t in tt],
                  'peak_allocated_MB': round(peak[1] / 1e6, 1)},
        'speedup_vs_torch': round(mt / mk, 2),
        'peak_allocated_MB': round(peak[0] / 1e6, 1),
        'windows': windows, 'steps': steps, 'batch': B, 'graph_step': False,
        'outputs_dropout_off': check,
        'workload': f'NGCF {U - 1:,} users x {I - 1:,} items, {len(u):,} edges (scale {scale}), '
                    f'64 / [64, 64, 64], message dropout 0.1, BPR + EmbLoss, FusedAdam',
        'dtype': 'fp32', 'data': 'synthetic (Zipf items, Zipf-like user degrees, seeded)',
        'setup_s': round(setup, 1),
        'note': f'first measurement: {windows} alternating windows of {steps} steps in one '
                f'process; no repeat across processes, spread beyond the windows not measured',
    }


def _criteo_fields(scale):
    """The C4 shape's fields for a StubDataset: (vocab, types, nums) of 13 float and 26 token
    fields."""
    from recbole_amd.utils import FeatureType
    vocab = [max(3, int(v * scale)) for v in c4_vocab()]
    types, nums = {'label': FeatureType.FLOAT}, {'label': 1}
    for j in range(13):
        types[f'I{j}'], nums[f'I{j}'] = FeatureType.FLOAT, 1
    for j, v in enumerate(vocab):
        types[f'C{j}'], nums[f'C{j}'] = FeatureType.TOKEN, v + 1
    return vocab, types, nums


def _criteo_batches(vocab, B, n_batches, dev):
    """Seeded batches of that shape on the device: log-normal floats scaled to [0, 1],
    Zipf(1.1) ids."""
    from recbole_amd.data.interaction import Interaction
    rng = np.random.default_rng(2020)
    batches = []
    for _ in range(n_batches):
        cols = {'label': torch.as_tensor((rng.random(B) < 0.256).astype(np.float32))}
        for j in range(13):
            x = rng.lognormal(0.0, 2.0, B)
            cols[f'I{j}'] = torch.as_tensor(((x - x.min()) / (x.max() - x.min())).astype(
                np.float32))
        for j, v in enumerate(vocab):
            cols[f'C{j}'] = torch.as_tensor(_zipf_ids(rng, 1.1, B, v))
        batches.append(Interaction(cols).to(dev))
    return batches


def bench_xdeepfm(dev, steps, warmup, scale=1.0, B=2048, d=16, n_batches=8, windows=3):
    """X4: one xDeepFM training step (zero_grad, calculate_loss, backward, FusedAdam with the
    [V, d] token table deferred) at the C4 shape with the reference's defaults
    (cin_layer_size [100, 100, 100], direct False, MLP 128-128-128-1, dropout 0.2, reg_weight
    5e-4): cin_kernel 'fused' (K18) against 'library' (the reference's op sequence) on copies
    of the same initial weights and the same batches. `windows` timed windows of `steps`
    steps each, the two sides alternating; peak allocated memory of each side's windows; the
    two steps' loss and CIN weight gradients compared on the first batch with the dropout
    off. K18's launches are timed by HIP events on their stream over eager steps."""
    import copy
    from recbole_amd.config import Config
    from recbole_amd.model.context_aware_recommender import xDeepFM
    from recbole_amd.trainer.optim import FusedAdam
    vocab, types, nums = _criteo_fields(scale)
    config = Config(model='xDeepFM', dataset='criteo-synth', config_dict={
        'embedding_size': d, 'load_col': None, 'state': 'ERROR', 'data_path': ROOT,
        'cin_kernel': 'fused'})
    config['device'] = dev
    torch.manual_seed(2020)
    model = xDeepFM(config, StubDataset(types, nums)).to(dev)
    twin = copy.deepcopy(model)
    twin.cin_kernel = 'library'
    batches = _criteo_batches(vocab, B, n_batches, dev)
    m = model.num_feature_field
    assert model.cin_fused_applies(torch.empty(B, m, d, device=dev))

    # the two steps' outputs on the first batch, dropout off
    check = {}
    for side, mod in (('fused', model), ('library', twin)):
        mod.dropout_prob = 0.0
        for q in mod.mlp_layers.mlp_layers:
            if isinstance(q, torch.nn.Dropout):
                q.p = 0.0
        mod.mlp_layers.dropout = 0.0
        loss = mod.calculate_loss(batches[0])
        loss.backward()
        check[f'loss_{side}'] = loss.item()
    check['loss_rel_diff'] = abs(check['loss_fused'] - check['loss_library']) / abs(
        check['loss_library'])
    check['grad_max_abs_diff'], check['grad_max_abs_library'] = {}, {}
    for (name, a), (_, b) in zip(model.named_parameters(), twin.named_parameters()):
        if name.startswith(('conv1d_list', 'cin_linear', 'mlp_layers')):
            check['grad_max_abs_diff'][name] = float((a.grad - b.grad).abs().max())
            check['grad_max_abs_library'][name] = float(b.grad.abs().max())
    for mod in (model, twin):
        mod.zero_grad(set_to_none=True)
        mod.dropout_prob = 0.2
        for q in mod.mlp_layers.mlp_layers:
            if isinstance(q, torch.nn.Dropout):
                q.p = 0.2
        mod.mlp_layers.dropout = 0.2

    opts = []
    for mod in (model, twin):
        opt = FusedAdam(mod.parameters(), lr=1e-3)
        if ADAM_MODE == 'deferred':
            opt.enable_deferred(mod.deferred_tables())
        opts.append(opt)
    it = [0, 0]

    def stepper(side, mod, opt):
        def step():
            b = batches[it[side] % n_batches]
            it[side] += 1
            opt.zero_grad()
            mod.calculate_loss(b).backward()
            opt.step()
        return step

    step_f, step_l = stepper(0, model, opts[0]), stepper(1, twin, opts[1])
    tf, tl, peak = [], [], [0, 0]
    for w in range(windows):
        for side, (fn, ts) in enumerate(((step_f, tf), (step_l, tl))):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            ts.append(_timed(fn, steps, warmup if w == 0 else 1, opts[side]))
            peak[side] = max(peak[side], torch.cuda.max_memory_allocated(dev))
    mf, ml = float(np.median(tf)), float(np.median(tl))
    resident = torch.cuda.memory_allocated(dev)
    ev = _window_events(step_f, ('cin_fwd', 'cin_bwd', 'cin_wgrad'))
    opts[0].flush()
    # FLOPs of one pass over the three layers: 2 N K per (sample, dimension) row
    layer_flops = [2 * B * d * N * H * m for H, N, _, _, _ in model.cin_plan]
    kern = {}
    for name, mult in (('cin_fwd', 1), ('cin_bwd', 2), ('cin_wgrad', 1)):
        n, us = ev[name]
        fl = mult * sum(layer_flops) / len(layer_flops)          # mean per launch
        kern[name] = {'launches_per_step': n, 'launch_us': round(us, 2),
                      'flops_per_launch': fl, 'bound': 'mfma',
                      'achieved': round(fl / (us * 1e-6) / 1e12, 2), 'unit': 'TFLOP/s',
                      'peak': MFMA_F32_PEAK_TFLOPS,
                      'frac': round(fl / (us * 1e-6) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                      'timing': 'HIP events around each launch on its stream, 8 eager steps; '
                                'cin_bwd counts the T = G W product and its two contractions '
                                'as 2 N K each; the finish launch after cin_wgrad is outside its pair'}
    spread = lambda ts: (max(ts) - min(ts)) / float(np.median(ts))
    V = sum(nums[f'C{j}'] for j in range(26))
    return {
        'config': 'X4', 'model': 'xDeepFM', 'metric': 'train samples/s (cin_kernel fused)',
        'value': round(B / mf, 1), 'unit': 'samples/s', 'ms_per_step': round(mf * 1e3, 3),
        'ms_per_step_windows': [round(t * 1e3, 3) for t in tf],
        'window_spread': round(spread(tf), 4),
        'peak_allocated_MB': round(peak[0] / 1e6, 1),
        'library': {'ms_per_step': round(ml * 1e3, 3), 'samples_per_s': round(B / ml, 1),
                    'ms_per_step_windows': [round(t * 1e3, 3) for t in tl],
                    'window_spread': round(spread(tl), 4),
                    'peak_allocated_MB': round(peak[1] / 1e6, 1)},
        'resident_MB_both_models': round(resident / 1e6, 1),
        'speedup_vs_library': round(ml / mf, 3),
        'fused_faster_beyond_spread': bool(max(tf) < min(tl)),
        'k18': kern, 'roofline': kern['cin_fwd'],
        'windows': windows, 'steps': steps, 'batch': B, 'graph_step': False,
        'adam_mode': ADAM_MODE, 'outputs_dropout_off': check,
        'workload': f'xDeepFM Criteo-shape: 13 float + 26 token fields, vocab {V:,} (incl. '
                    f'PADs), d={d}, CIN [100, 100, 100] direct False, MLP {m * d}-128-128-128-1, '
                    f'dropout 0.2, reg_weight 5e-4, BCE, FusedAdam',
        'dtype': 'fp32', 'data': 'synthetic (Zipf(1.1) ids, log-normal floats, seeded)',
        'note': f'first measurement: {windows} alternating windows of {steps} steps in one '
                f'process; no repeat across processes',
    }


def _set_dropout(mod, p):
    mod.dropout_prob = p
    mod.mlp_layers.dropout = p
    for q in mod.mlp_layers.mlp_layers:
        if isinstance(q, torch.nn.Dropout):
            q.p = p


def bench_dcn(dev, steps, warmup, scale=1.0, B=2048, d=16, n_batches=8, windows=3):
    """D4: one DCN training step (zero_grad, calculate_loss, backward, FusedAdam with the
    [V, d] token table deferred) at the C4 shape with the reference's defaults (6 cross layers,
    MLP 256-256-256 with BatchNorm, dropout 0.2, reg_weight 2): cross_kernel 'fused' (K19)
    against 'library' (the reference's op sequence, cat and predict_layer) on copies of the
    same initial weights and the same batches. `windows` timed windows of `steps` steps each,
    the two sides alternating; peak allocated memory of each side's windows; the two steps'
    loss and gradients compared on the first batch with the dropout off. K19's two launches
    are timed by HIP events on their stream over eager steps."""
    import copy
    from recbole_amd.config import Config
    from recbole_amd.model.context_aware_recommender import DCN
    from recbole_amd.trainer.optim import FusedAdam
    vocab, types, nums = _criteo_fields(scale)
    config = Config(model='DCN', dataset='criteo-synth', config_dict={
        'embedding_size': d, 'load_col': None, 'state': 'ERROR', 'data_path': ROOT,
        'cross_kernel': 'fused'})
    config['device'] = dev
    torch.manual_seed(2020)
    model = DCN(config, StubDataset(types, nums)).to(dev)
    twin = copy.deepcopy(model)
    twin.cross_kernel = 'library'
    batches = _criteo_batches(vocab, B, n_batches, dev)
    n, L = model.num_feature_field * d, model.cross_layer_num
    assert model.cross_fused_applies(torch.empty(B, n, device=dev))
    assert not twin.cross_fused_applies(torch.empty(B, n, device=dev))

    # the two steps' outputs on the first batch, dropout off
    check = {}
    for side, mod in (('fused', model), ('library', twin)):
        _set_dropout(mod, 0.0)
        loss = mod.calculate_loss(batches[0])
        loss.backward()
        check[f'loss_{side}'] = loss.item()
    check['loss_rel_diff'] = abs(check['loss_fused'] - check['loss_library']) / abs(
        check['loss_library'])
    check['grad_max_abs_diff'], check['grad_max_abs_library'] = {}, {}
    for (name, a), (_, b) in zip(model.named_parameters(), twin.named_parameters()):
        if name.startswith(('cross_layer', 'predict_layer', 'float_embedding_table')):
            check['grad_max_abs_diff'][name] = float((a.grad - b.grad).abs().max())
            check['grad_max_abs_library'][name] = float(b.grad.abs().max())
    for mod in (model, twin):
        mod.zero_grad(set_to_none=True)
        _set_dropout(mod, 0.2)
        for q in mod.mlp_layers.mlp_layers:          # the comparison step's statistics: undone
            if isinstance(q, torch.nn.BatchNorm1d):
                q.reset_running_stats()

    opts = []
    for mod in (model, twin):
        opt = FusedAdam(mod.parameters(), lr=1e-3)
        if ADAM_MODE == 'deferred':
            opt.enable_deferred(mod.deferred_tables())
        opts.append(opt)
    it = [0, 0]

    def stepper(side, mod, opt):
        def step():
            b = batches[it[side] % n_batches]
            it[side] += 1
            opt.zero_grad()
            mod.calculate_loss(b).backward()
            opt.step()
        return step

    step_f, step_l = stepper(0, model, opts[0]), stepper(1, twin, opts[1])
    tf, tl, peak = [], [], [0, 0]
    for w in range(windows):
        for side, (fn, ts) in enumerate(((step_f, tf), (step_l, tl))):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            ts.append(_timed(fn, steps, warmup if w == 0 else 1, opts[side]))
            peak[side] = max(peak[side], torch.cuda.max_memory_allocated(dev))
    mf, ml = float(np.median(tf)), float(np.median(tl))
    resident = torch.cuda.memory_allocated(dev)
    ev = _window_events(step_f, ('cross_fwd', 'cross_bwd'))
    opts[0].flush()
    # bytes a launch has to move: x0 in (and dx0 out), the parameters, S, y / gy
    moved = {'cross_fwd': 4 * (B * n + 2 * L * n + n + B * L + B),
             'cross_bwd': 4 * (2 * B * n + 2 * L * n + n + B * L + B)}
    kern = {}
    for name in ('cross_fwd', 'cross_bwd'):
        cnt, us = ev[name]
        kern[name] = {'launches_per_step': cnt, 'launch_us': round(us, 2),
                      'bytes_per_launch': moved[name], 'bound': 'latency / launch',
                      'achieved': round(moved[name] / (us * 1e-6) / 1e9, 1), 'unit': 'GB/s',
                      'timing': 'HIP events around each launch on its stream, 8 eager steps; '
                                'the finish launch after cross_bwd is outside its pair'}
    spread = lambda ts: (max(ts) - min(ts)) / float(np.median(ts))
    V = sum(nums[f'C{j}'] for j in range(26))
    return {
        'config': 'D4', 'model': 'DCN', 'metric': 'train samples/s (cross_kernel fused)',
        'value': round(B / mf, 1), 'unit': 'samples/s', 'ms_per_step': round(mf * 1e3, 3),
        'ms_per_step_windows': [round(t * 1e3, 3) for t in tf],
        'window_spread': round(spread(tf), 4),
        'peak_allocated_MB': round(peak[0] / 1e6, 1),
        'library': {'ms_per_step': round(ml * 1e3, 3), 'samples_per_s': round(B / ml, 1),
                    'ms_per_step_windows': [round(t * 1e3, 3) for t in tl],
                    'window_spread': round(spread(tl), 4),
                    'peak_allocated_MB': round(peak[1] / 1e6, 1)},
        'resident_MB_both_models': round(resident / 1e6, 1),
        'speedup_vs_library': round(ml / mf, 3),
        'fused_faster_beyond_spread': bool(max(tf) < min(tl)),
        'k19': kern, 'roofline': kern['cross_bwd'],
        'windows': windows, 'steps': steps, 'batch': B, 'graph_step': False,
        'adam_mode': ADAM_MODE, 'outputs_dropout_off': check,
        'workload': f'DCN Criteo-shape: 13 float + 26 token fields, vocab {V:,} (incl. PADs), '
                    f'd={d}, n={n}, {L} cross layers, MLP {n}-256-256-256 with BatchNorm, '
                    f'dropout 0.2, reg_weight 2, BCE, FusedAdam',
        'dtype': 'fp32', 'data': 'synthetic (Zipf(1.1) ids, log-normal floats, seeded)',
        'note': f'first measurement: {windows} alternating windows of {steps} steps in one '
                f'process; no repeat across processes',
    }


def bench_afm(dev, steps, warmup, scale=1.0, B=2048, d=16, n_batches=8, windows=3):
    """A4: one AFM training step (zero_grad, calculate_loss, backward, FusedAdam with the
    [V, d] and [V, 1] token tables deferred) at the C4 field shape with the reference's
    defaults (attention_size 25, dropout 0.3, reg_weight 2): afm_kernel 'fused' (K20) against
    'library' (the reference's op sequence: the [B, P, d] and [B, P, A] pair tensors in
    memory) on copies of the same initial weights and the same batches. `windows` timed
    windows of `steps` steps each, the two sides alternating; each side's peak allocated
    memory above what was resident when its window began (the models, optimizer states and
    batches); the two steps' loss and gradients compared on the first batch with the dropout
    off. K20's two launches are timed by HIP events on their stream over eager steps."""
    import copy
    from recbole_amd.config import Config
    from recbole_amd.model.context_aware_recommender import AFM
    from recbole_amd.trainer.optim import FusedAdam
    vocab, types, nums = _criteo_fields(scale)
    config = Config(model='AFM', dataset='criteo-synth', config_dict={
        'embedding_size': d, 'load_col': None, 'state': 'ERROR', 'data_path': ROOT,
        'afm_kernel': 'fused'})
    config['device'] = dev
    torch.manual_seed(2020)
    model = AFM(config, StubDataset(types, nums)).to(dev)
    twin = copy.deepcopy(model)
    twin.afm_kernel = 'library'
    batches = _criteo_batches(vocab, B, n_batches, dev)
    F, A, p_drop = model.num_feature_field, model.attention_size, model.dropout_prob
    P = F * (F - 1) // 2
    assert model.afm_fused_applies(torch.empty(B, F, d, device=dev))
    assert not twin.afm_fused_applies(torch.empty(B, F, d, device=dev))

    def set_dropout(mod, p):
        mod.dropout_prob = p
        mod.dropout_layer.p = p

    # the two steps' outputs on the first batch, dropout off
    check = {}
    for side, mod in (('fused', model), ('library', twin)):
        set_dropout(mod, 0.0)
        loss = mod.calculate_loss(batches[0])
        loss.backward()
        check[f'loss_{side}'] = loss.item()
    check['loss_rel_diff'] = abs(check['loss_fused'] - check['loss_library']) / abs(
        check['loss_library'])
    check['grad_max_abs_diff'], check['grad_max_abs_library'] = {}, {}
    for (name, a), (_, b) in zip(model.named_parameters(), twin.named_parameters()):
        if name.startswith(('attlayer', 'p', 'float_embedding_table')):
            check['grad_max_abs_diff'][name] = float((a.grad - b.grad).abs().max())
            check['grad_max_abs_library'][name] = float(b.grad.abs().max())
    for mod in (model, twin):
        mod.zero_grad(set_to_none=True)
        set_dropout(mod, p_drop)

    opts = []
    for mod in (model, twin):
        opt = FusedAdam(mod.parameters(), lr=1e-3)
        if ADAM_MODE == 'deferred':
            opt.enable_deferred(mod.deferred_tables())
        opts.append(opt)
    it = [0, 0]

    def stepper(side, mod, opt):
        def step():
            b = batches[it[side] % n_batches]
            it[side] += 1
            opt.zero_grad()
            mod.calculate_loss(b).backward()
            opt.step()
        return step

    step_f, step_l = stepper(0, model, opts[0]), stepper(1, twin, opts[1])
    tf, tl, peak = [], [], [0, 0]
    for w in range(windows):
        for side, (fn, ts) in enumerate(((step_f, tf), (step_l, tl))):
            torch.cuda.synchronize()
            opts[side].zero_grad()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            ts.append(_timed(fn, steps, warmup if w == 0 else 1, opts[side]))
            peak[side] = max(peak[side], torch.cuda.max_memory_allocated(dev) - base)
    mf, ml = float(np.median(tf)), float(np.median(tl))
    resident = torch.cuda.memory_allocated(dev)
    ev = _window_events(step_f, ('afm_fwd', 'afm_bwd'))
    opts[0].flush()
    # the MFMA work of a launch as K20 walks it: slabs of 16 pair rows with one left field,
    # d and A padded to 16; forward one product, backward four (u twice, W^T du, du^T z)
    slabs = sum((F - 1 - i + 15) // 16 for i in range(F - 1))
    dp, apad = (d + 15) // 16 * 16, (A + 15) // 16 * 16
    per = 2 * 16 * dp * apad * slabs * B
    flops = {'afm_fwd': per, 'afm_bwd': 4 * per}
    useful = 2 * P * d * A * B
    kern = {}
    for name in ('afm_fwd', 'afm_bwd'):
        cnt, us = ev[name]
        tf_s = flops[name] / (us * 1e-6) / 1e12
        kern[name] = {'launches_per_step': cnt, 'launch_us': round(us, 2),
                      'mfma_flop_per_launch': flops[name],
                      'useful_flop_per_product': useful,
                      'achieved': round(tf_s, 2), 'unit': 'TFLOP/s (padded MFMA work)',
                      'fraction_of_fp32_mfma_peak': round(tf_s / MFMA_F32_PEAK_TFLOPS, 4),
                      'timing': 'HIP events around each launch on its stream, 8 eager steps; '
                                'the finish launch after afm_bwd is outside its pair'}
    spread = lambda ts: (max(ts) - min(ts)) / float(np.median(ts))
    V = sum(nums[f'C{j}'] for j in range(26))
    return {
        'config': 'A4', 'model': 'AFM', 'metric': 'train samples/s (afm_kernel fused)',
        'value': round(B / mf, 1), 'unit': 'samples/s', 'ms_per_step': round(mf * 1e3, 3),
        'ms_per_step_windows': [round(t * 1e3, 3) for t in tf],
        'window_spread': round(spread(tf), 4),
        'peak_above_resident_MB': round(peak[0] / 1e6, 1),
        'library': {'ms_per_step': round(ml * 1e3, 3), 'samples_per_s': round(B / ml, 1),
                    'ms_per_step_windows': [round(t * 1e3, 3) for t in tl],
                    'window_spread': round(spread(tl), 4),
                    'peak_above_resident_MB': round(peak[1] / 1e6, 1)},
        'resident_MB_both_models': round(resident / 1e6, 1),
        'speedup_vs_library': round(ml / mf, 3),
        'fused_faster_beyond_spread': bool(max(tf) < min(tl)),
        'k20': kern, 'roofline': kern['afm_bwd'],
        'windows': windows, 'steps': steps, 'batch': B, 'graph_step': False,
        'adam_mode': ADAM_MODE, 'outputs_dropout_off': check,
        'workload': f'AFM Criteo-shape: 13 float + 26 token fields, vocab {V:,} (incl. PADs), '
                    f'd={d}, F={F}, P={P} pairs ({slabs} slabs), attention_size {A}, dropout '
                    f'{p_drop}, reg_weight 2, BCE, FusedAdam',
        'dtype': 'fp32', 'data': 'synthetic (Zipf(1.1) ids, log-normal floats, seeded)',
        'note': f'first measurement: {windows} alternating windows of {steps} steps in one '
                f'process; no repeat across processes',
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C3,C4,C5')
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--scale', type=float, default=1.0)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--adam-mode', default='deferred', choices=['deferred', 'streamed'])
    ap.add_argument('--eager-step', action='store_true', help='C3 / C4 without the captured step')
    ap.add_argument('--c3-loss', default='SSM', choices=list(C3_LOSSES),
                    help='C3 loss: sampled softmax (default) or the full-catalogue cross '
                         'entropy on the library path / on K12')
    ap.add_argument('--c3-model', default='SASRec', choices=['SASRec', 'GRU4Rec'],
                    help='the sequential model of the C3-shaped step')
    args = ap.parse_args()
    global CPU_BASELINE, ADAM_MODE, GRAPH_STEP
    CPU_BASELINE = not args.no_cpu_baseline
    GRAPH_STEP = not args.eager_step
    ADAM_MODE = args.adam_mode
    dev = torch.device('cuda', 0)
    res = []
    for c in args.configs.split(','):
        if c == 'C3' and args.c3_model == 'GRU4Rec':
            r = bench_c3_gru4rec(dev, args.steps, args.warmup, args.scale, loss=args.c3_loss)
        elif c == 'C3':
            r = bench_c3(dev, args.steps, args.warmup, args.scale, loss=args.c3_loss)
        elif c == 'C4':
            r = bench_c4(dev, args.steps, args.warmup, args.scale)
        elif c == 'C5':
            r = bench_c5(dev, args.scale)
        elif c == 'N2':
            r = bench_neumf(dev, args.steps, args.warmup, args.scale)
        elif c == 'A2':
            r = bench_multivae(dev, args.steps, args.warmup, args.scale)
        elif c == 'G2':
            r = bench_ngcf(dev, args.steps, args.warmup, args.scale)
        elif c == 'B3':
            r = bench_bert4rec(dev, args.steps, args.warmup, args.scale)
        elif c in ('X4', 'xDeepFM'):
            r = bench_xdeepfm(dev, args.steps, args.warmup, args.scale)
        elif c in ('D4', 'DCN'):
            r = bench_dcn(dev, args.steps, args.warmup, args.scale)
        elif c in ('A4', 'AFM'):
            r = bench_afm(dev, args.steps, args.warmup, args.scale)
        else:
            raise SystemExit(f'unknown config {c}')
        print(json.dumps(r), flush=True)
        res.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
