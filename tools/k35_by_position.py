"""K35 by position in its chunk, from a rocprofv3 kernel trace of plain `python bench.py`.

The K35 launches (bpr_adam_step_kernel) of the run are split into chunks at the closing
flushes (adam_flush_scan_kernel / adam_flush_row_kernel); per chunk: launches, span from the
first launch's start to the last one's end, the sum of the durations, the mean duration;
for the steady 64-step chunks each launch's duration at positions 0-7, 28-35 and 56-63;
and the closing flushes (FG), the background flushes (BG: adam_flush_walk_kernel) and the
advance launches (ADV: adam_flush_first_kernel) in time order, each foreground launch with the
gap since the previous foreground launch of the list ended.

usage: python tools/k35_by_position.py <trace dir> [label]
"""
import csv
import glob
import sys

import numpy as np

RANGES = ((0, 8), (28, 36), (56, 64))


def load(src):
    path = sorted(glob.glob(f'{src}/**/*kernel_trace.csv', recursive=True))[0]
    rows = [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'])
            for r in csv.DictReader(open(path))]
    return sorted(rows)


def chunks_of(rows):
    """[[(start, end)] per chunk], [(kind, start, end)] of the flush launches."""
    chunks, cur, flushes = [], [], []
    for s, e, name in rows:
        if 'bpr_adam_step_kernel' in name:
            cur.append((s, e))
        elif 'adam_flush_scan_kernel' in name or 'adam_flush_row_kernel' in name:
            flushes.append(('FG', s, e))
            if cur:
                chunks.append(cur)
                cur = []
        elif 'adam_flush_walk_kernel' in name:
            flushes.append(('BG', s, e))
        elif 'adam_flush_first_kernel' in name:
            flushes.append(('ADV', s, e))
    if cur:
        chunks.append(cur)
    return chunks, flushes


def main(src, label=''):
    chunks, flushes = chunks_of(load(src))
    t0 = chunks[0][0][0]
    us = lambda t: t / 1e3
    print(f'# {label}: microseconds; t = from the first K35 launch of the run')
    print('## chunks (split at the closing flushes)')
    for i, c in enumerate(chunks):
        d = np.array([e - s for s, e in c]) / 1e3
        span = us(c[-1][1] - c[0][0])
        print(f'chunk {i}: K35 x {len(c):3d}  t={us(c[0][0] - t0):9.1f}  span={span:8.1f}  '
              f'sum={d.sum():8.1f}  idle={span - d.sum():7.1f}  mean={d.mean():6.2f}  '
              f'min={d.min():6.2f}  max={d.max():6.2f}')
    steady = [(i, c) for i, c in enumerate(chunks) if len(c) == 64][1:]   # [0] is the warm-up
    print('## K35 duration by position, steady 64-step chunks')
    for lo, hi in RANGES:
        for i, c in steady:
            d = [us(e - s) for s, e in c[lo:hi]]
            print(f'chunk {i} pos {lo:2d}-{hi - 1:2d}: ' + ' '.join(f'{x:6.2f}' for x in d) +
                  f'   mean {np.mean(d):6.2f}')
    print('## mean by eighth of the chunk (positions 8k .. 8k+7), one row per steady chunk')
    for i, c in steady:
        d = np.array([us(e - s) for s, e in c]).reshape(8, 8).mean(axis=1)
        print(f'chunk {i}: ' + ' '.join(f'{x:6.2f}' for x in d))
    print('## flush launches')
    prev = None
    for kind, s, e in flushes:
        if s >= t0:
            gap = f'  gap={us(s - prev):6.1f}' if prev is not None and kind != 'BG' else ''
            print(f'{kind:3s} t={us(s - t0):9.1f} dur={us(e - s):7.1f}{gap}')
            if kind != 'BG':
                prev = e


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else '')
