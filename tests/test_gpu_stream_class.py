"""The two classes of stream the library makes (lanefront_core.h, StreamClass): the live map's has the greatest priority where the
device has a range, a handle's the normal one -- between the two ends, never the map's -- whichever of them was made first; where
the device has one priority, both report it.  (Handles at the LEAST priority were built first: that class has a pool of hardware
queues of its own, but ran the flagship pipeline 10 % slower -- DESIGN.md section 5 -- so the handles stay normal and are dealt
evenly by idle streams made in front of the first one.  Which hardware queue a stream lands on is not visible through HIP: the placement is
shown by a kernel trace, tools/chain_gaps.py.)"""
import pytest
import torch                                         # before the library: INTEGRATION.md, fourth note

from lane_slam_amd import FrontEnd, LineAssociator, default_config

pytestmark = pytest.mark.gpu


def _handle():
    return FrontEnd(default_config("parity", in_size=(120, 160)), max_frames=3, max_lines_per_color=256)


def test_the_map_greatest_and_the_handles_alike():
    assert torch.cuda.is_available()
    before = _handle()
    a = LineAssociator(capacity=4096)
    after = _handle()
    try:
        p_before, least, greatest = before.stream_priority()
        p_map, m_least, m_greatest = a.stream_priority()
        p_after, a_least, a_greatest = after.stream_priority()
        assert (least, greatest) == (m_least, m_greatest) == (a_least, a_greatest)
        if least != greatest:
            assert p_map == greatest
            # (HIP counts priorities downwards: the greatest is the smallest number)
            assert min(least, greatest) <= p_before <= max(least, greatest) and p_before != greatest
            assert p_before == 0                     # the normal priority, that of a plain hipStreamCreate
        else:
            assert p_before == p_map == p_after == least
        assert p_before == p_after                   # made before the map or after it: the same class
        # (the getters take null pointers for what the caller does not ask)
        assert before.lib.lf_stream_priority(before.h, None, None, None) == 0
        assert a.lib.lf_map_stream_priority(a.m, None, None, None) == 0
    finally:
        a.close()
        before.close()
        after.close()
