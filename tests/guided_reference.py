"""numpy float32 restatement of the guided estimate and a replay of a guided frame's session.

A plain module (no tests): tests/test_guided_reference.py and tests/test_gpu_guided.py import it.  The guided block
error is by definition k_adaptive_error of what k_temporal_accumulate would output, so it is written exactly so:
temporal_reference.accumulate, then the block estimate in the kernel's op order.  Nothing here uses GPU output."""
import numpy as np

import temporal_reference as tref
from denoise_reference import F32, bits


def block_error(film, mom, W, H, abs_floor):
    """k_adaptive_error: E per image-aligned 8x8 block [rows, columns], float32.  Per pixel with n >= 2: mean = s / n,
    d = fmax(q - s mean, 0), sem = sqrt((d / (n - 1)) / n), else both 0; both summed over the block's 64 lanes (lane l =
    pixel (l % 8, l // 8) of the block, 0 outside the image) by the xor butterfly, offsets 32 .. 1;
    E = S / (M + abs_floor)."""
    film, mom = np.asarray(film, F32).reshape(W * H, 4), np.asarray(mom, F32).reshape(W * H, 2)
    nbx, nby = (W + 7) // 8, (H + 7) // 8
    n, s, q = film[:, 3], mom[:, 0], mom[:, 1]
    ok = n >= F32(2)
    with np.errstate(all="ignore"):
        mean = s / n
        d = np.fmax(q - s * mean, F32(0))
        sem = np.sqrt((d / (n - F32(1))) / n)
    mean = np.where(ok, mean, F32(0)).astype(F32)
    sem = np.where(ok, sem, F32(0)).astype(F32)

    def lanes(v):
        img = np.zeros((nby * 8, nbx * 8), F32)
        img[:H, :W] = v.reshape(H, W)
        return img.reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3).reshape(nby, nbx, 64)

    def butterfly(v):
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[..., idx ^ o]).astype(F32)
        return v[..., 0]
    S, M = butterfly(lanes(sem)), butterfly(lanes(mean))
    with np.errstate(all="ignore"):
        return (S / (M + F32(abs_floor))).astype(F32)


def guided_block_error(film, mom, feat, pos, history, M, W, H, abs_floor, **desc):
    """rt_temporal_block_error: the block errors of the film and moments accumulated against `history` (None: none)."""
    return block_error(*tref.accumulate(film, mom, feat, pos, history, M, W, H, **desc)[:2], W, H, abs_floor)


def simulate_frame(levels, feat, pos, history, M, W, H, min_samples, step_samples, max_samples, rel_error, abs_floor,
                   estimate=None, owned=None, **desc):
    """A guided frame's adaptive session replayed on uniform films.  levels[k] = (film, mom) of a uniform session that
    stopped at k indices, for every k the session can stop at (min_samples, then + step_samples, clipped to
    max_samples).  All owned pixels (owned: a bool mask, default all) start at min_samples; each iteration takes the
    guided block errors of the composed film; the pixels of converged blocks freeze, the rest move to the next level.
    estimate(film, mom) -> E [rows, columns] replaces the numpy estimate (the GPU's, in tests/test_gpu_guided.py).
    Returns dict(film, mom, active = the active pixel count after each iteration, samples = the sample total,
    iterations, index_done, block_error = the last estimate [rows, columns]): the fields of rt_adaptive_info are
    iterations, index_done, active_pixels = active[-1], active_blocks = the open blocks of block_error, samples."""
    N = W * H
    if estimate is None:
        def estimate(f, m):
            return guided_block_error(f, m, feat, pos, history, M, W, H, abs_floor, **desc)
    y, x = np.divmod(np.arange(N), W)
    block = (y // 8) * ((W + 7) // 8) + x // 8
    active = np.ones(N, bool) if owned is None else np.asarray(owned, bool).copy()
    film, mom = np.zeros((N, 4), F32), np.zeros((N, 2), F32)
    done, counts, samples = 0, [], 0
    E = np.zeros(((H + 7) // 8, (W + 7) // 8), F32)
    while active.any() and done < max_samples:
        nxt = min(max_samples, done + (min_samples if not counts else step_samples))
        samples += int(active.sum()) * (nxt - done)
        done = nxt
        film[active], mom[active] = levels[done][0][active], levels[done][1][active]
        E = estimate(film, mom)
        conv = (E <= F32(rel_error)).reshape(-1)
        active &= ~conv[block]
        counts.append(int(active.sum()))
    return dict(film=film, mom=mom, active=counts, samples=samples, iterations=len(counts), index_done=done,
                block_error=E)
