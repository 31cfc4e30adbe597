"""The stream-order model (tests/stream_model.py) on hand-written forests with known answers.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc  # noqa: E402
import stream_model as sm  # noqa: E402


def test_a_single_chain_is_order_one():
    path = [(x, 2) for x in range(9)] + [(8, 3), (7, 4)]
    dirs = sc.paint(sc.blank(6, 10), path)
    chan = sc.mask_of(dirs.shape, path)
    order = sm.stream_order(dirs, 255, chan)
    assert np.array_equal(order, chan)                      # 1 on the chain, 0 elsewhere
    kinds = sm.stream_links(dirs, order, 255, chan)
    assert kinds[2, 0] == sm.HEAD and kinds[4, 7] == sm.MOUTH and (kinds[2, 1:9] == sm.PLAIN).all()


def test_a_perfect_binary_tree_of_depth_k_has_order_k_at_its_root():
    for k in range(1, 8):
        dirs, root, cells = sc.binary_tree(k, ox=1, oy=1)
        for chan in (None, sc.mask_of(dirs.shape, cells)):
            order = sm.stream_order(dirs, 255, chan)
            assert order[root[1], root[0]] == k
            assert order.max() == k
            kinds = sm.stream_links(dirs, order, 255, chan)
            assert (kinds == sm.ORDER_STEP).sum() == 0
            if chan is not None:
                assert (kinds == sm.HEAD).sum() == 2 ** (k - 1) and (kinds == sm.JUNCTION).sum() == 2 ** (k - 1) - 1


def test_three_equal_orders_give_one_more_not_two_more():
    dirs = sc.three_way(8, 8, (18, 18))
    order = sm.stream_order(dirs)
    assert order[8, 7] == 2 and order[7, 8] == 2 and order[8, 9] == 2
    assert order[8, 8] == 3
    dirs = sc.blank(5, 5)                                   # three heads into one cell
    dirs[2, 1], dirs[1, 2], dirs[2, 3] = 5, 7, 1
    assert sm.stream_order(dirs)[2, 2] == 2


def test_a_junction_of_orders_2_1_1_stays_2():
    dirs = sc.blank(8, 8)
    sc.paint(dirs, [(1, 1), (2, 2), (3, 3), (4, 4)], last=None)      # becomes order 2 at (2, 2)
    dirs[1, 2] = 7                                                    # (2, 1) -> (2, 2): the second head
    dirs[4, 3] = 5                                                    # (3, 4) -> (4, 4): order 1
    dirs[3, 4] = 7                                                    # (4, 3) -> (4, 4): order 1
    order = sm.stream_order(dirs)
    assert order[2, 2] == 2 and order[3, 3] == 2 and order[4, 3] == 1 and order[3, 4] == 1
    assert order[4, 4] == 2


def test_a_loop_is_255_and_what_drains_into_it_is_finite():
    """Every cell has ONE target, so nothing lies downstream of a loop but the loop itself: the "tail" of this case is a
    second feeder.  The queue never releases the four loop cells; the tributary (with a junction) and the feeder are trees."""
    dirs, loop, feeders = sc.loop_with_tributary(8, 5, (16, 20))
    order = sm.stream_order(dirs)
    for x, y in loop:
        assert order[y, x] == 255
    assert (order == 255).sum() == 4
    assert order[5, 3] == 1 and order[3, 5] == 1 and order[4, 5] == 1 and order[5, 5] == 2 and order[5, 7] == 2
    for x, y in feeders:
        assert 1 <= order[y, x] <= 2
    kinds = sm.stream_links(dirs, order)
    assert kinds[5, 8] == sm.JUNCTION and (kinds == sm.ORDER_STEP).sum() == 0


def test_a_mask_that_is_not_closed_downstream_ends_the_tree():
    path = [(x, 1) for x in range(10)]
    dirs = sc.paint(sc.blank(4, 10), path)
    dirs[0, 6] = 7                                          # a head into (6, 1), below the gap
    dirs[2, 1] = 3                                          # a head into (1, 1), above the gap
    chan = np.ones(dirs.shape, np.uint8)
    chan[1, 3] = 0                                          # the gap
    chan[3, :] = 0
    order = sm.stream_order(dirs, 255, chan)
    assert list(order[1]) == [1, 2, 2, 0, 1, 1, 2, 2, 2, 2]
    kinds = sm.stream_links(dirs, order, 255, chan)
    assert kinds[1, 2] == sm.MOUTH and kinds[1, 4] == sm.HEAD and kinds[1, 3] == 0
    assert (sm.stream_order(dirs, 255, None)[1] == [1, 2, 2, 2, 2, 2, 2, 2, 2, 2]).all()


def test_nodata_cells_are_zero_for_any_nodata_code():
    dirs = sc.paint(sc.blank(3, 6), [(x, 1) for x in range(6)])
    dirs[1, 2] = 7                                          # the NoData code of this raster: 7 is no direction here
    order = sm.stream_order(dirs, 7)
    assert list(order[1]) == [1, 1, 0, 1, 1, 1] and order[0, 0] == 1


def test_channels_threshold():
    acc = np.array([[-1.0, 1.0, 5.0], [4.999, 100.0, -1.0]])
    assert np.array_equal(sm.channels(acc, 5.0), np.array([[0, 0, 1], [0, 1, 0]], np.uint8))


def test_the_python_layer_exports_the_entries():
    import richdem_amd as rd

    for name in ("d8_channels", "d8_stream_order", "d8_stream_links", "d8_channels_dev", "d8_stream_order_dev",
                 "d8_stream_links_dev"):
        assert callable(getattr(rd, name)) and name in rd.__all__
