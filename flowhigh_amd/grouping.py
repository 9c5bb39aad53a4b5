"""How generate_many cuts a list of clips into launch sequences: pure list logic, no GPU (tests/test_grouping_cpu.py)."""


def plan_buckets(lengths, rates, shapes, streams, max_batch, steps=None):
    """The batches of the bucketed path -> (number of streams used, [(stream index, input rate, clip indices), ...] in launch
    order).  Clips of one (length, rate, noise shape) are one bucket, in list order, cut into parts of at most max_batch
    clips.  The per-shape workspaces are keyed by (batch, frames), so every bucket of one frame count (shape[1]) runs on one
    stream: the distinct frame counts, ascending, take the `streams` streams round-robin.
    steps: None, or one step count per clip; the count then joins the bucket's key (a batch runs one count)."""
    buckets = {}
    for i, key in enumerate(zip(lengths, rates, shapes, steps if steps is not None else [None] * len(lengths))):
        buckets.setdefault(key, []).append(i)
    frame_counts = sorted({shape[1] for _, _, shape, _ in buckets})
    n_streams = max(1, min(int(streams), len(frame_counts)))
    stream_of = {n: i % n_streams for i, n in enumerate(frame_counts)}
    return n_streams, [(stream_of[shape[1]], rate, idx[k:k + max_batch])
                       for (_, rate, shape, _), idx in buckets.items() for k in range(0, len(idx), max_batch)]


def pack_ragged(frames, width, max_frames, chunk_limit):
    """Greedy packing of the ragged path, in list order -> (groups, alone): clip i is width[i] rows of frames[i] frames, a
    group holds at most max_frames frames over its rows.  alone: the clips that fit no sequence (more than max_frames frames
    of their own, or more than chunk_limit > 0 frames in a row: the vocoder would chunk them).  A group of one is still a
    group; the caller runs it as it runs the clips of `alone`."""
    groups, alone, cur, tot = [], [], [], 0
    for i, (n, w) in enumerate(zip(frames, width)):
        if n * w > max_frames or (chunk_limit > 0 and n > chunk_limit):
            alone.append(i)
            continue
        if cur and tot + n * w > max_frames:
            groups.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += n * w
    if cur:
        groups.append(cur)
    return groups, alone
