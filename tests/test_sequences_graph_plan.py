"""The conditions on the generator of tests/sequence_graph_ops.py, asserted on the CPU: every kept sequence (the usable seeds of
range(60)) is replayed on the oracle alone, and what the replays did is counted.  The op probabilities of the helper are set so
that these hold; a condition is never loosened to fit them."""
import functools

import sequence_graph_ops as ops


@functools.lru_cache(maxsize=None)
def measured():
    return ops.measure(ops.seeds(60))


def test_every_op_kind_occurs_often_enough_on_each_graph_form():
    m = measured()
    print(m)
    for kind, name in ops.NEW_OPS.items():
        assert m["sequences_with"][kind] >= 8, f"op {kind} ({name}) occurs in {m['sequences_with'][kind]} sequences"
        assert m["sparse_times"][kind] >= 3 or kind == 7, f"op {kind} ({name}) on sparse handles"      # (7: dense handles only)
        assert m["dense_times"][kind] >= 3, f"op {kind} ({name}) on dense handles"
    assert m["sparse_times"][7] == 0


def test_structural_ops_change_column_counts_before_a_run():
    assert measured()["structural_then_run"] >= 10


def test_few_writing_ops_are_void():
    m = measured()
    assert m["writes"] > 0 and m["voids"] <= 0.2 * m["writes"], (m["voids"], m["writes"])


def test_edge_lists_stay_installed_across_structural_ops_on_sparse_handles():
    assert measured()["list_across_structural"] >= 5


def test_some_sparse_connect_call_holds_two_records_for_one_block():
    """(the later record wins: connect_rule applies them in order to the oracle's matrices)"""
    assert measured()["repeated_blocks"] >= 1


def test_the_docstring_counts_are_the_measured_ones():
    assert measured() == ops.MEASURED, ("the generator draws other sequences than its docstring describes (draw(), the op table or an "
                                        "op changed): if every condition above still holds, update MEASURED in sequence_graph_ops.py and "
                                        f"the counts in its docstring to {measured()}")
    for n in (ops.MEASURED["writes"], ops.MEASURED["sequences"]):
        assert str(n) in ops.__doc__


def test_a_sequence_is_a_function_of_its_seed():
    seed = ops.seeds(60)[0]
    assert ops.play(None, seed, device=False)[0] == ops.play(None, seed, device=False)[0]
