"""The host-only parts of the edge-weight history: the façade's assembly of the one recorder list and the slicing of its result
(lattice.edge_history_plan), and the history object (lattice.EdgeHistory: len, [t], .edges, .dense()).  No GPU."""
import numpy as np
import pytest

from snn_amd import lattice
from snn_amd.lattice import EdgeHistory, GraphPosition, edge_history_plan


def test_plan_concatenates_and_slices():
    a = ("connecting", [7, 8, 9], [0, 1, 2], 1)
    b = (3, np.array([4, 5], np.int64), np.array([5, 4], np.int64), 2)
    pre, post, when, columns = edge_history_plan([a, b])
    assert pre.dtype == np.uint32 and post.dtype == np.uint32 and when.dtype == np.uint8
    assert pre.tolist() == [7, 8, 9, 4, 5] and post.tolist() == [0, 1, 2, 5, 4] and when.tolist() == [1, 1, 1, 2, 2]
    assert columns == {"connecting": slice(0, 3), 3: slice(3, 5)}
    result = np.arange(20, dtype=np.float32).reshape(4, 5)          # [steps, n] as the device returns it
    assert result[:, columns[3]].tolist() == [[3, 4], [8, 9], [13, 14], [18, 19]]
    # an empty segment keeps its (empty) slice; no segment at all gives empty lists of the right types
    pre, post, when, columns = edge_history_plan([("connecting", [], [], 1), (0, [1], [2], 2)])
    assert columns == {"connecting": slice(0, 0), 0: slice(0, 1)} and pre.tolist() == [1] and when.tolist() == [2]
    pre, post, when, columns = edge_history_plan([])
    assert pre.size == post.size == when.size == 0 and pre.dtype == np.uint32 and columns == {}


def test_plan_refuses_what_the_device_would_not_take():
    with pytest.raises(ValueError):
        edge_history_plan([("connecting", [1, 2], [3], 1)])
    with pytest.raises(ValueError):
        edge_history_plan([("connecting", [1], [3], 3)])


def history():
    weights = np.array([[1.0, 0.0, 0.5], [1.5, 0.0, 0.0], [2.0, 0.25, 0.0]], np.float32)
    connected = np.array([[True, False, True], [True, False, True], [True, True, False]])
    return weights, connected


def test_connecting_history_object():
    weights, connected = history()
    keys = [(GraphPosition(0, (i, 0)), GraphPosition(1, (0, 0))) for i in range(3)]
    built = []
    h = EdgeHistory(lambda: built.append(1) or keys, weights, connected)
    assert len(h) == 3 and not built                              # the keys are built when they are first asked for
    assert h[0] == {keys[0]: 1.0, keys[2]: 0.5}
    assert h[1] == {keys[0]: 1.5, keys[2]: 0.0}                   # Some(0.0) stays, None is left out
    assert h[-1] == {keys[0]: 2.0, keys[1]: 0.25}
    assert h.edges is keys and built == [1]
    assert [len(step) for step in h] == [2, 2, 2]
    with pytest.raises(TypeError):
        h.dense()
    with pytest.raises(IndexError):
        h[3]


def test_lattice_history_object_and_dense():
    weights, connected = history()
    pre, post = np.array([0, 2, 1]), np.array([1, 0, 1])
    h = EdgeHistory(list(zip(pre.tolist(), post.tolist())), weights, connected, pre, post, 3)
    assert h.edges == [(0, 1), (2, 0), (1, 1)] and h[2] == {(0, 1): 2.0, (2, 0): 0.25}
    dense = h.dense()
    assert dense.shape == (3, 3, 3) and dense.dtype == np.float32
    want = np.zeros((3, 3, 3), np.float32)
    want[:, 0, 1] = [1.0, 1.5, 2.0]
    want[:, 2, 0] = [0.0, 0.0, 0.25]
    want[:, 1, 1] = [0.5, 0.0, 0.0]
    assert np.array_equal(dense, want)
    empty = EdgeHistory([], np.zeros((0, 0), np.float32), np.zeros((0, 0), bool), np.zeros(0, int), np.zeros(0, int), 2)
    assert len(empty) == 0 and empty.dense().shape == (0, 2, 2)


def test_the_host_container_resets_graph_histories():
    net = lattice.LatticeNetwork()
    l = lattice.Lattice(4)
    net.add_lattice(l)
    l.weights_history = np.ones((2, 0, 0), np.float32)
    net.connecting_graph_history = EdgeHistory([], np.zeros((5, 0), np.float32), np.zeros((5, 0), bool))
    assert len(net.connecting_graph_history) == 5
    net.reset_graph_history()
    assert len(net.connecting_graph_history) == 0 and l.weights_history.shape[0] == 0
