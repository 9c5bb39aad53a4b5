"""GPU: the 24-bit encoders -- fh_pcm_s24_f32, fh_pcm_s24_seg_f32 and fh_stream_pcm_s24_rows_f32 against flowhigh_amd/pcm.py
(quantize24, pack24), bit for bit.

The encoder does exact or correctly rounded operations (one float64 product that is exact, one float64 add, rint), so every test
is an equality.  A packed sample is 3 bytes and rows, clips and blocks abut at any byte address, so every output lies between 64
guard bytes of 0xA5 that must keep their value, and the segment form's clips are packed back to back with no padding: a store
wider than the row, or a read-modify-write of a shared word, would show in a neighbour."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import hip, pcm                                         # noqa: E402
from flowhigh_amd.frontend import upload_tables                            # noqa: E402

GUARD = 64
SENT = 0xA5
LSB = 2.0 ** -23
LENS = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 2047, 2048, 2049, 4097]      # 2048 samples: one block's span
EDGES = np.array([1.0, -1.0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 2.0 ** -24, -2.0 ** -24, 0.5 * LSB, -0.5 * LSB, 1.5 * LSB, -1.5 * LSB,
                  2.5 * LSB, -2.5 * LSB, 0.0, -0.0, np.nan, np.inf, -np.inf, 1.5, -1.5, 1e-40, -1e-40], dtype=np.float32)
KEYS = [(77 + 2 ** 33, 5), (2 ** 64 - 1, 0), (3, 2 ** 40)]
_WANT = {}


def st():
    return hip.stream()


def planted(n_clips, C, T, seed):
    """Uniform on (-1.05, 1.05), a third of it scaled to a few LSB (there the dither decides), the edge values planted over it."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.05, 1.05, (n_clips, C, T)).astype(np.float32)
    flat = x.reshape(-1)
    flat[::3] *= np.float32(4 * LSB)
    pos = rng.permutation(flat.size)[:EDGES.size]
    flat[pos] = np.roll(EDGES, seed)[:pos.size]
    return x


def dev_keys(keys):
    return torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64)).cuda()


def want_bytes(x, key, interleaved, container):
    """One clip [C, T] -> the bytes of its encoding as uint8 [container * C * T]."""
    q = pcm.encode24(x, key, bool(interleaved), packed=container == 3)
    return torch.from_numpy(np.ascontiguousarray(q).reshape(-1).view(np.uint8).copy())


def framed(n_bytes, offset):
    """A uint8 buffer of 0xA5 whose part [GUARD + offset, + n_bytes) is the output; the buffer itself is 256-byte aligned."""
    buf = torch.full((GUARD + offset + n_bytes + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + offset:GUARD + offset + n_bytes]


def intact(buf, offset, n_bytes):
    lo = GUARD + offset
    return bool((buf[:lo] == SENT).all()) and bool((buf[lo + n_bytes:] == SENT).all())


def source(x, shift):
    """x on the device, its first float `shift` floats past a 16-byte boundary."""
    buf = torch.full((x.size + 8,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    xd = buf[shift:shift + x.size]
    xd.copy_(torch.from_numpy(x.reshape(-1)))
    return buf, xd


def clip_case(C, T, n_clips):
    """The inputs of a shape and what every (layout, dither, container) of them encodes to, made once."""
    k = (C, T, n_clips)
    if k not in _WANT:
        x = planted(n_clips, C, T, seed=T + 10 * C + n_clips)
        _WANT[k] = x, {(i, d, B): torch.cat([want_bytes(x[b], KEYS[b] if d else None, i, B) for b in range(n_clips)])
                       for i in (0, 1) for d in (False, True) for B in (3, 4)}
    return _WANT[k]


# ---- the batched entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_clips", [1, 3])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_batched_entry_gives_pcm_py_s_bits(C, n_clips):
    """Every length either side of a run of 8, of a wave and of a block, planar and interleaved, with and without dither, both
    containers; the packed output at byte offsets 0 .. 3 (the int32 one at 0 and 4), the source 0 .. 3 floats past a 16-byte
    boundary (so the 16-byte and the 4-byte loads both run); 64 guard bytes either side keep their 0xA5."""
    L = hip.lib()
    kd = dev_keys(KEYS[:n_clips])
    for T in LENS:
        x, wants = clip_case(C, T, n_clips)
        n = x.size
        for shift in range(4):
            keep, xd = source(x, shift)
            for B in (3, 4):
                offset = shift if B == 3 else 4 * (shift & 1)
                for interleaved in (0, 1):
                    for dither in (False, True):
                        buf, y = framed(B * n, offset)
                        hip.check(L.fh_pcm_s24_f32(xd.data_ptr(), y.data_ptr(), kd.data_ptr() if dither else 0, n_clips, C, T,
                                                   interleaved, B, st()), "fh_pcm_s24_f32")
                        case = (T, shift, B, interleaved, dither)
                        assert torch.equal(y.cpu(), wants[interleaved, dither, B]), case
                        assert intact(buf, offset, B * n), case


def test_containers_hold_the_same_integer_and_dither_is_the_channel_s_own():
    """pack24 of the int32 result is the packed result; channel 1 of a clip in a batch of 4-channel clips is channel 1 of a
    2-channel clip alone under the same key, planar or interleaved; channel 0 is not channel 1."""
    L = hip.lib()
    T, key = 777, (123456789, 42)
    x = (planted(3, 4, T, seed=5) * np.float32(3 * LSB)).astype(np.float32)      # a few LSB: the dither decides most samples
    x = np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
    kd, xd = dev_keys([(1, 1), (2, 2), key]), torch.from_numpy(x).cuda()
    wide = torch.empty(3, 4, T, dtype=torch.int32, device="cuda")
    packed = torch.empty(3, 4, T, 3, dtype=torch.uint8, device="cuda")
    hip.check(L.fh_pcm_s24_f32(xd.data_ptr(), wide.data_ptr(), kd.data_ptr(), 3, 4, T, 0, 4, st()), "fh_pcm_s24_f32")
    hip.check(L.fh_pcm_s24_f32(xd.data_ptr(), packed.data_ptr(), kd.data_ptr(), 3, 4, T, 0, 3, st()), "fh_pcm_s24_f32")
    assert np.array_equal(pcm.pack24(wide.cpu().numpy()), packed.cpu().numpy())
    pair, k1 = torch.from_numpy(np.ascontiguousarray(x[2, :2])).cuda(), dev_keys([key])
    y2 = torch.empty(T, 2, dtype=torch.int32, device="cuda")
    hip.check(L.fh_pcm_s24_f32(pair.data_ptr(), y2.data_ptr(), k1.data_ptr(), 1, 2, T, 1, 4, st()), "fh_pcm_s24_f32")
    assert torch.equal(y2.t().cpu(), wide[2, :2].cpu())
    same = torch.from_numpy(np.stack([x[2, 0], x[2, 0]])).cuda()
    y3 = torch.empty(2, T, dtype=torch.int32, device="cuda")
    hip.check(L.fh_pcm_s24_f32(same.data_ptr(), y3.data_ptr(), k1.data_ptr(), 1, 2, T, 0, 4, st()), "fh_pcm_s24_f32")
    assert not torch.equal(y3[0], y3[1])


# ---- the segment entry ---------------------------------------------------------------------------------------------------------
SEG_SHAPES = [(1, 1), (9, 3), (2049, 2), (7, 8), (33, 1), (5, 2), (2047, 3), (3, 1)]          # (len, C)


@pytest.mark.parametrize("container", [3, 4])
@pytest.mark.parametrize("interleaved", [0, 1])
@pytest.mark.parametrize("dither", [False, True])
def test_segment_entry_gives_every_clip_the_bits_of_the_batched_entry(dither, interleaved, container):
    """Clips of different (len, C) in one launch, their outputs back to back with no padding at byte offset 1 (packed: neighbours
    share words), the second clip's rows 13 floats apart in a wider buffer: each equal to fh_pcm_s24_f32 on that clip alone with
    its key, and to pcm.py.  Clips with 0 or 9 channels or no samples, pointing into the guard, are left unwritten."""
    L = hip.lib()
    B = container
    keys = [(9, i) for i in range(len(SEG_SHAPES))]
    xs = [planted(1, c, t, seed=40 + t)[0] for t, c in SEG_SHAPES]
    pitches = [t if i != 1 else 13 for i, (t, c) in enumerate(SEG_SHAPES)]
    srcs, alone = [], []
    for x, (t, c), pitch, key in zip(xs, SEG_SHAPES, pitches, keys):
        wide = torch.full((c, pitch), float("nan"))
        wide[:, :t] = torch.from_numpy(x)
        srcs.append(wide.cuda())
        y = torch.empty(B * c * t, dtype=torch.uint8, device="cuda")
        xd, k1 = torch.from_numpy(x).cuda(), dev_keys([key])
        hip.check(L.fh_pcm_s24_f32(xd.data_ptr(), y.data_ptr(), k1.data_ptr() if dither else 0, 1, c, t, interleaved, B, st()),
                  "fh_pcm_s24_f32")
        alone.append(y.cpu())
        assert torch.equal(alone[-1], want_bytes(x, key if dither else None, interleaved, B))
    sizes = [B * t * c for t, c in SEG_SHAPES]
    off = [int(o) for o in np.cumsum([0] + sizes[:-1])]
    offset = 1 if B == 3 else 4
    buf, y = framed(sum(sizes), offset)
    clips = [hip.PcmClip(s.data_ptr(), y.data_ptr() + o, p, c, t) for s, o, p, (t, c) in zip(srcs, off, pitches, SEG_SHAPES)]
    # what must write nothing: its dst is the guard in front of the output
    bad = [hip.PcmClip(srcs[2].data_ptr(), buf.data_ptr(), 2049, 0, 2049), hip.PcmClip(srcs[2].data_ptr(), buf.data_ptr(), 100, 9, 100),
           hip.PcmClip(srcs[2].data_ptr(), buf.data_ptr(), 2049, 2, 0)]
    table = clips[:3] + bad + clips[3:]
    all_keys = keys[:3] + [(1, 1)] * 3 + keys[3:]
    keep, (tp,) = upload_tables([(hip.PcmClip * len(table))(*table)], torch.device("cuda"))
    kd = dev_keys(all_keys)
    hip.check(L.fh_pcm_s24_seg_f32(tp, len(table), 8, 2049, kd.data_ptr() if dither else 0, interleaved, B, st()), "fh_pcm_s24_seg_f32")
    got = y.cpu()
    for i, (o, n) in enumerate(zip(off, sizes)):
        assert torch.equal(got[o:o + n], alone[i]), (i, SEG_SHAPES[i])
    assert intact(buf, offset, sum(sizes))


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    L = hip.lib()
    x = torch.zeros(64, device="cuda")
    buf, y = framed(4 * 64, 0)
    table = (hip.PcmClip * 1)(hip.PcmClip(x.data_ptr(), y.data_ptr(), 64, 1, 64))
    keep, (tp, gp) = upload_tables([table, np.array([0, 1], dtype=np.int32)], torch.device("cuda"))
    jobs = (hip.StreamJob * 1)(hip.StreamJob(0, x.data_ptr(), y.data_ptr(), 0, 0, 0, 0, 64, 64, 0, 0, 0))
    keep2, (jp,) = upload_tables([jobs], torch.device("cuda"))
    s = st()
    bad = [("fh_pcm_s24_f32", (x.data_ptr(), y.data_ptr(), 0, 1, 1, 64, 0, 2, s), "container"),
           ("fh_pcm_s24_f32", (x.data_ptr(), y.data_ptr(), 0, 1, 1, 64, 0, 5, s), "container"),
           ("fh_pcm_s24_f32", (x.data_ptr(), y.data_ptr(), 0, 1, 1, 64, 0, 0, s), "container"),
           ("fh_pcm_s24_f32", (x.data_ptr(), y.data_ptr() + 1, 0, 1, 1, 63, 0, 4, s), "4-byte"),
           ("fh_pcm_s24_f32", (x.data_ptr(), y.data_ptr() + 2, 0, 1, 1, 63, 1, 4, s), "4-byte"),
           ("fh_pcm_s24_f32", (0, y.data_ptr(), 0, 1, 1, 64, 0, 3, s), "null"),
           ("fh_pcm_s24_f32", (x.data_ptr(), y.data_ptr(), 0, 1, 9, 7, 0, 3, s), "channels"),
           ("fh_pcm_s24_f32", (x.data_ptr(), y.data_ptr(), 0, 1, 1, 0, 0, 3, s), "len"),
           ("fh_pcm_s24_seg_f32", (tp, 1, 1, 64, 0, 0, 6, s), "container"),
           ("fh_pcm_s24_seg_f32", (0, 1, 1, 64, 0, 0, 3, s), "null"),
           ("fh_pcm_s24_seg_f32", (tp, 1, 9, 64, 0, 0, 3, s), "channels"),
           ("fh_stream_pcm_s24_rows_f32", (jp, 1, gp, 1, 64, 0, 0, 1, s), "container"),
           ("fh_stream_pcm_s24_rows_f32", (0, 1, gp, 1, 64, 0, 0, 3, s), "null"),
           ("fh_stream_pcm_s24_rows_f32", (jp, 1, 0, 1, 64, 0, 0, 3, s), "null")]
    for entry, args, word in bad:
        assert getattr(L, entry)(*args) != 0, (entry, args)
        said = L.fh_last_error().decode()
        assert entry in said and word in said, (entry, said)
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    # a table's clip with a misaligned int32 dst is left unwritten
    table = (hip.PcmClip * 1)(hip.PcmClip(x.data_ptr(), y.data_ptr() + 2, 60, 1, 60))
    keep, (tp,) = upload_tables([table], torch.device("cuda"))
    hip.check(L.fh_pcm_s24_seg_f32(tp, 1, 1, 60, 0, 0, 4, s), "fh_pcm_s24_seg_f32")
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ---- the streaming entry -------------------------------------------------------------------------------------------------------
BLOCKS = (1, 7, 8, 9, 2047, 2049, 0, 333)


def launch_rows(jobs, groups, max_out, keys, frames, container):
    keep, (jp, gp) = upload_tables([(hip.StreamJob * len(jobs))(*jobs), np.asarray(groups, dtype=np.int32)], torch.device("cuda"))
    rc = hip.lib().fh_stream_pcm_s24_rows_f32(jp, len(jobs), gp, len(groups) - 1, max_out, keys, frames, container, st())
    torch.cuda.synchronize()
    return rc


def block_jobs(rows, a, n, dsts, first):
    """One job per row: the block rows[:, a:a + n] fresh, nothing carried, its first sample the absolute index first + a."""
    return [hip.StreamJob(0, rows[c, a:].data_ptr() if n else 0, dsts[c] if n else 0, 0, first + a, first + a, 0, n, n, 0, 0, 0)
            for c in range(rows.shape[0])]


@pytest.mark.parametrize("container", [3, 4])
@pytest.mark.parametrize("frames", [0, 1])
@pytest.mark.parametrize("first", [0, 2 ** 32 + 5])
def test_stream_blocks_add_up_to_the_batched_entry(first, frames, container):
    """A mono and a 3-channel stream in one launch per block, blocks of 1, 7, 8, 9, 2047, 2049, 0 and 333 samples with `first`
    running on (from 0, and from past 2^32): every block lands where it belongs in the stream's output buffer -- packed blocks
    abut at any byte address -- and the whole equals fh_pcm_s24_f32 on the whole stream (from 0) and pcm.py (from anywhere)."""
    L = hip.lib()
    B, T = container, sum(BLOCKS)
    keys = [(77, 0), (5, 2 ** 40)]
    xs = [planted(1, C, T, seed=60 + C)[0] for C in (1, 3)]
    devs = [torch.from_numpy(x).cuda() for x in xs]
    offset = 3 if B == 3 else 4
    outs = [framed(B * x.size, offset) for x in xs]
    kd = dev_keys(keys)
    a = 0
    for n in BLOCKS:
        jobs = []
        for x, (buf, y) in zip(devs, outs):
            C = x.shape[0]
            if frames:
                dsts = [y.data_ptr() + B * a * C] * C
            else:
                dsts = [y.data_ptr() + B * (c * T + a) for c in range(C)]
            jobs += block_jobs(x, a, n, dsts, first)
        assert launch_rows(jobs, [0, 1, 4], n, kd.data_ptr(), frames, B) == 0
        a += n
    for x, xd, (buf, y), key in zip(xs, devs, outs, keys):
        C = x.shape[0]
        d = np.stack([pcm.tpdf_dither(key[0], key[1], c, T, first=first) for c in range(C)])
        q = pcm.quantize24(x, d)
        q = np.ascontiguousarray(q.T) if frames else q
        want = (pcm.pack24(q) if B == 3 else q).reshape(-1).view(np.uint8)
        assert np.array_equal(y.cpu().numpy(), want), (C, first)
        assert intact(buf, offset, B * x.size)
        if first == 0:
            whole = torch.empty(B * x.size, dtype=torch.uint8, device="cuda")
            hip.check(L.fh_pcm_s24_f32(xd.data_ptr(), whole.data_ptr(), dev_keys([key]).data_ptr(), 1, C, T, frames, B, st()), "fh_pcm_s24_f32")
            assert torch.equal(whole, y)


@pytest.mark.parametrize("container", [3, 4])
@pytest.mark.parametrize("frames", [0, 1])
def test_bad_groups_are_left_unwritten(frames, container):
    """A group with a null dst, one with unequal counters, one of 9 jobs and (int32) one with a misaligned dst write nothing; the
    good group beside them is written, without dither too."""
    B, n = container, 100
    x = torch.from_numpy(planted(1, 3, n, seed=3)[0]).cuda()
    buf, y = framed(B * 3 * n, 0)
    scratch, z = framed(B * 16 * n, 0)

    def rows(k, at, **over):
        js = block_jobs(x[:1].expand(k, n) if k > 3 else x[:k], 0, n, [at + (0 if frames else B * c * n) for c in range(k)], 0)
        for name, (c, v) in over.items():
            setattr(js[c], name, v)
        return js
    jobs = rows(3, y.data_ptr())                                                             # the good one
    jobs += rows(2, z.data_ptr(), dst=(0 if frames else 1, 0))                                # a null dst it would use
    jobs += rows(2, z.data_ptr(), first=(1, 8))                                               # unequal counters
    jobs += rows(9, z.data_ptr())                                                             # too many rows
    groups = [0, 3, 5, 7, 16]
    if B == 4:
        jobs += rows(2, z.data_ptr() + 2)                                                     # int32 at 2 mod 4
        groups.append(18)
    assert launch_rows(jobs, groups, n, 0, frames, B) == 0
    assert bool((scratch == SENT).all()) and intact(buf, 0, B * 3 * n)
    assert torch.equal(y.cpu(), want_bytes(x.cpu().numpy(), None, frames, B))
