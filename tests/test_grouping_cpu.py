"""CPU: how generate_many cuts a list of clips into ragged groups and buckets (flowhigh_amd/grouping.py).  The packing cases
are the ones tests/test_hip_ragged_ends.py and tests/test_hip_level.py run on the device: frame counts 50 131 20 50 220 77 5."""
from flowhigh_amd.grouping import pack_ragged, plan_buckets

FRAMES = [50, 131, 20, 50, 220, 77, 5]


def test_packing_is_greedy_in_list_order_and_a_long_clip_runs_alone():
    assert pack_ragged(FRAMES, [1] * 7, 200, 6000) == ([[0, 1], [2, 3, 5, 6]], [4])


def test_a_group_of_one_is_still_a_group():
    """max_frames = 131: 50 + 131 does not fit, 131 fills a group, 220 fits none."""
    assert pack_ragged(FRAMES, [1] * 7, 131, 6000) == ([[0], [1], [2, 3], [5, 6]], [4])


def test_a_clip_counts_its_channels_times_its_frames():
    assert pack_ragged([50, 50, 30], [2, 1, 8], 200, 6000) == ([[0, 1]], [2])              # 30 * 8 > 200
    assert pack_ragged([50, 50, 30], [2, 1, 8], 240, 6000) == ([[0, 1], [2]], [])          # 150 + 240 > 240: a group of its own


def test_a_clip_the_vocoder_would_chunk_runs_alone_whatever_max_frames_is():
    for max_frames in (50, 80, 12000):
        groups, alone = pack_ragged([30, 50], [1, 1], max_frames, 40)
        assert alone == [1] and groups == [[0]]
    assert pack_ragged([30, 50], [1, 1], 12000, 0) == ([[0, 1]], [])                       # chunk_limit = 0: no such rule
    assert pack_ragged([], [], 200, 6000) == ([], [])


def test_buckets_are_keyed_by_length_rate_and_noise_shape():
    n, parts = plan_buckets([6000, 6000, 6000], [12000, 12000, 16000], [(1, 50, 256), (2, 50, 256), (1, 37, 256)], 1, 64)
    assert n == 1 and parts == [(0, 12000, [0]), (0, 12000, [1]), (0, 16000, [2])]


def test_equal_frame_counts_share_a_stream():
    """6000 and 6001 samples at 12 kHz are 50 frames both (one workspace): one stream; streams=3 over two frame counts uses two."""
    shapes = [(1, 50, 256), (1, 50, 256), (1, 20, 256), (1, 50, 256)]
    n, parts = plan_buckets([6000, 6001, 2400, 6000], [12000] * 4, shapes, 3, 64)
    assert n == 2
    assert parts == [(1, 12000, [0, 3]), (1, 12000, [1]), (0, 12000, [2])]                 # (frame counts ascending: 20 -> 0, 50 -> 1)
    assert plan_buckets([6000, 6001, 2400, 6000], [12000] * 4, shapes, 1, 64)[0] == 1
    assert plan_buckets([6000, 6001, 2400, 6000], [12000] * 4, shapes, 0, 64)[0] == 1      # (never fewer than one)


def test_a_bucket_splits_into_parts_of_max_batch_clips_in_order():
    n, parts = plan_buckets([6000] * 5, [12000] * 5, [(1, 50, 256)] * 5, 1, 2)
    assert [p for _, _, p in parts] == [[0, 1], [2, 3], [4]]
    mixed = plan_buckets([6000, 2400, 6000, 6000], [12000] * 4, [(1, 50, 256), (1, 20, 256), (1, 50, 256), (1, 50, 256)], 1, 2)[1]
    assert [p for _, _, p in mixed] == [[0, 2], [3], [1]]                                  # (buckets in the order their first clip came)
