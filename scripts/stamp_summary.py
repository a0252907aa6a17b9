"""Summarise FG_STAMP s_memtime stamps (diagnostic builds): per stage, for the wave of
group 0 and of group 1 on one SIMD: memory section (t1-t0), barrier wait into the compute
section (t2-t1), compute issue (t3-t2), barrier wait out (t4-t3); cycles.  Then the per-tile
stamps of wave 0, and for raw launches that stage their records the epilogue split: pretest
with staging, commit, fallback walk, and the share of tiles in which the walk ran."""
import sys
import numpy as np

a = np.fromfile(sys.argv[1], dtype=np.uint64)[:16 * 2 * 2 * 32 * 6].reshape(16, 2, 2, 32, 6).astype(np.int64)
ok = (a[..., 0] > 0) & (a[..., 4] > 0)
for g in range(2):
    sel = a[:, :, g][ok[:, :, g]]
    d = np.diff(sel, axis=-1)
    per = np.diff(sel[:, 0])
    print(f"group {g}: n={len(sel)}  mem {np.median(d[:, 0]):.0f}  wait-in {np.median(d[:, 1]):.0f}  "
          f"mfma {np.median(d[:, 2]):.0f}  wait-out {np.median(d[:, 3]):.0f}  (median cycles; total "
          f"{np.median(d.sum(-1)):.0f})")

# per-tile stamps (wave 0 of workgroups 0..63, tiles 0..15): setup start, setup barrier
# passed, K loop done, fast-path test done, slow path done, flush barrier passed, flush /
# epilogue done.  A stamp the tile did not pass (no uniform test, no flush barrier) is
# filled from its predecessor, so that part reads 0.
t8 = np.fromfile(sys.argv[1], dtype=np.uint64)[16384:16384 + 64 * 128].reshape(64, 16, 8).astype(np.int64)
# Raw launches with staged records: slot 7 is the commit's end (0 in a tile without survivors)
# and slot 5 the start of the fallback walk, written only in tiles where it ran.
staged = bool((t8[..., 7] > 0).any())
t7 = np.where(t8[..., 7] > 0, t8[..., 7], t8[..., 3])
walked = t8[..., 5] > 0
t = t8[..., :7].copy()
if staged:
    t[..., 5] = 0
for k in range(3, 6):
    t[..., k] = np.where(t[..., k] > 0, t[..., k], t[..., k - 1])
okt = (t[..., 0] > 0) & (t[..., 6] > 0)
sel = t[okt]
if len(sel):
    d = np.diff(sel, axis=-1)
    gap = (t[:, 1:, 0] - t[:, :-1, 6])[okt[:, 1:] & okt[:, :-1]]
    mgap = np.median(gap) if len(gap) else 0
    epi = sel[:, 6] - sel[:, 2]
    tot = np.median(sel[:, 6] - sel[:, 0]) + mgap
    print(f"tiles: n={len(sel)}  setup {np.median(d[:, 0]):.0f}  K loop {np.median(d[:, 1]):.0f}  "
          f"epilogue {np.median(epi):.0f}  gap to next {mgap:.0f}  "
          f"(median s_memtime ticks; K loop share {np.median(d[:, 1]) / tot:.3f})")
    names = ["fast-path test", "slow path", "flush barrier wait", "flush"]
    print("epilogue of wave 0: " + "  ".join(
        f"{n} median {np.median(d[:, 2 + i]):.0f} mean {np.mean(d[:, 2 + i]):.0f}" for i, n in enumerate(names)))
    if staged:
        pre, com, walk = (sel[:, 3] - sel[:, 2]), (t7[okt] - sel[:, 3]), (sel[:, 4] - np.maximum(t7[okt], sel[:, 3]))
        print("raw epilogue of wave 0: " + "  ".join(
            f"{n} median {np.median(v):.0f} mean {np.mean(v):.0f}"
            for n, v in (("pretest + staging", pre), ("commit", com), ("fallback walk", walk)))
            + f"  fallback walk ran in {walked[okt].mean():.4f} of tiles")
    slow = d[:, 3] > 200   # wave 0 itself took the slow path
    print(f"  wave 0 took the slow path in {slow.mean():.2f} of tiles"
          + (f" (median {np.median(d[slow, 3]):.0f} there)" if slow.any() else "")
          + f"; tiles that flushed records: {(d[:, 5] > 200).mean():.2f}")
