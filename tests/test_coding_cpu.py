"""The host-side pieces the context-model coders share (clc_amd/models/coding.py) and the one container implementation behind
ans.split_pack / ans.lanes_pack, where no GPU is needed: the upload image of a device-decoded batch against a plain-loop restatement
(a split batch at n_state = 2, a lanes batch at n_state = 128, unequal lengths, one stream that is its state alone), the int32 refusal
from word counts alone, the end-state check under both nouns, the two containers' own magic and limits, and the one batch parser
over both.
"""
import numpy as np
import pytest
import torch


def _subs(counts, seed):
    g = np.random.default_rng(seed)
    return [[g.integers(0, 1 << 32, n, dtype=np.uint32).astype("<u4").tobytes() for n in img] for img in counts]


@pytest.mark.parametrize("n_state,counts", [(2, [[5, 2, 3], [4, 9, 2]]), (128, [[128, 141], [133, 130]])])
def test_upload_image_layout(n_state, counts):
    from clc_amd.models import coding

    subs = _subs(counts, n_state)
    B, S = len(counts), len(counts[0])
    assert any(n == n_state for img in counts for n in img)   # a stream with no word past its state
    # restated with plain loops
    state, spans, words, at = np.zeros((B, S, n_state + 2), np.uint32), np.zeros((B, S, 2), np.uint32), [], 0
    for b in range(B):
        for s in range(S):
            w = np.frombuffer(subs[b][s], dtype="<u4")
            for i in range(n_state):
                state[b, s, i] = w[i]
            state[b, s, n_state] = n_state   # pos: the next word to read
            state[b, s, n_state + 1] = 0     # pad
            spans[b, s] = (at, len(w))
            words += [int(v) for v in w]
            at += len(w)
    image = coding.stream_image(subs, n_state)
    assert image.dtype == np.int32 and image.shape == ((n_state + 4) * B * S + at,)
    got = coding.stream_views(image.view(np.uint32), B, S, n_state)
    assert got[0].shape == (B, S, n_state + 2) and got[1].shape == (B, S, 2)
    assert np.array_equal(got[0], state) and np.array_equal(got[1], spans) and got[2].tolist() == words
    assert int(got[1][0, 0, 0]) == 0 and (got[1].reshape(-1, 2)[1:, 0] == np.cumsum(got[1].reshape(-1, 2)[:-1, 1])).all()   # back to back
    # the same views of a tensor, as the upload takes them
    tv = coding.stream_views(torch.from_numpy(image), B, S, n_state)
    assert all(np.array_equal(t.numpy().view(np.uint32), a) for t, a in zip(tv, got))


def test_spans_refuse_what_int32_cannot_hold():
    from clc_amd.models import coding

    assert coding.stream_spans([3, 0, (1 << 31) - 4]).tolist() == [[0, 3], [3, 0], [3, (1 << 31) - 4]]
    for counts in ([1 << 31], [1 << 30, 1 << 30], [(1 << 31) - 1, 1]):
        with pytest.raises(ValueError, match=rf"decompress: {sum(counts)} stream words in one batch; the spans are int32"):
            coding.stream_spans(counts)


@pytest.mark.parametrize("noun,S,L", [("sub-stream", 3, 1), ("wave stream", 2, 64)])
def test_end_state_check(noun, S, L):
    from clc_amd.models import coding

    B = 3
    counts = np.arange(B * S).reshape(B, S) + 2 * L
    x = np.full((B, S, L), 1 << 31, dtype=np.uint64)
    coding.check_stream_ends(x, counts, counts, noun)   # every stream at its end: returns
    off = x.copy()
    off[1, S - 1, L - 1] += np.uint64(1 << 32)   # one state off, in image 1
    with pytest.raises(ValueError, match=rf"decompress: image 1: {noun}s \[{S - 1}\] did not decode to their end \({noun} {S - 1}: 1 of {L} states "
                                         rf"not at 2\^31, {counts[1, S - 1]} of {counts[1, S - 1]} words") as e:
        coding.check_stream_ends(off, counts, counts, noun)
    assert "image 0" not in str(e.value) and "image 2" not in str(e.value) and "corrupt, truncated" in str(e.value)
    short = counts.copy()
    short[2, 0] -= 1   # pos one short
    with pytest.raises(ValueError, match=rf"image 2: {noun}s \[0\] did not decode to their end .*{short[2, 0]} of {counts[2, 0]} words consumed"):
        coding.check_stream_ends(x, short, counts, noun)
    # the device coder's state tensor, (x low, x high) per state, pos, pad, reduces to the same input
    st = np.zeros((B, S, 2 * L + 2), dtype=np.uint32)
    st[..., 0:2 * L:2], st[..., 1:2 * L:2], st[..., 2 * L] = off & np.uint64(0xFFFFFFFF), off >> np.uint64(32), short
    xs, pos = coding.device_ends(torch.from_numpy(st.view(np.int32)))
    assert xs.dtype == np.uint64 and np.array_equal(xs, off) and np.array_equal(pos, short)


def test_container_parameterisation():
    """one implementation, two formats: each pair keeps its own magic, largest count and least length"""
    from clc_amd import ans

    from clc_amd.models import coding

    table = [(ans.split_pack, ans.split_unpack, ans.SPLIT_MAGIC, "S", 64, "sub-stream", 8, ans.SPLIT_STREAM, "substreams"),
             (ans.lanes_pack, ans.lanes_unpack, ans.LANES_MAGIC, "W", 16, "wave stream", 512, ans.LANES_STREAM, "lanes")]
    blobs = []
    for pack, unpack, magic, letter, most, noun, least, fmt, keyword in table:
        streams = [bytes([i]) * (least + 4 * i) for i in range(most)]
        blob = pack(streams)   # the largest count is accepted: S = 64 by split, W = 16 by lanes
        assert blob[:4] == magic and blob[4] == most and unpack(blob) == streams
        # the models' parser of a batch, one for both containers: the caller's keyword and the format's noun in its refusal
        assert coding.stream_parse(fmt, [blob, pack(streams[:2])][:1], most, keyword) == [streams]
        with pytest.raises(ValueError, match=rf"^decompress: {keyword} = {most}, but the header of image 1 says 2 {noun}s$"):
            coding.stream_parse(fmt, [blob, pack(streams[:2])], most, keyword)
        with pytest.raises(ValueError, match=rf"_pack: {letter} must be between 1 and {most} {noun}s \(got {most + 1}\)"):
            pack(streams + streams[:1])
        with pytest.raises(ValueError, match=rf"_pack: {noun} 1 has {least - 4} bytes; a length must be a multiple of 4 and at least {least}$"):
            pack([streams[0], streams[0][:-4]])
        blobs.append(blob)
    for (_, unpack, magic, *_), other in zip(table, reversed(blobs)):
        with pytest.raises(ValueError, match=rf"bad magic {other[:4]!r} \(.* starts with {magic!r}\)"):
            unpack(other)
    assert len(ans.split_unpack(blobs[0])) == 64
    with pytest.raises(ValueError, match=r"lanes_pack: W must be between 1 and 16 wave streams \(got 17\)"):
        ans.lanes_pack([bytes(512)] * 17)
    with pytest.raises(ValueError, match=r"lanes_unpack: W must be between 1 and 16 wave streams \(got 17\)"):   # split's 17 is not lanes'
        ans.lanes_unpack(ans.LANES_MAGIC + ans.split_pack([bytes(8)] * 17)[4:])
