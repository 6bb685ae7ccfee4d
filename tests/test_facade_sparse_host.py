"""Record-held blocks between lattices on the host (no GPU): with LatticeNetwork.hold_connecting_rules a connect(pre_id, post_id,
ConnectionRule, WeightRule) keeps the record instead of one dict entry per edge, and everything the class lets one read answers
exactly as the closure-built twin does -- the twin comparison of tests/test_connect_rule_host.py.  With the flag off nothing
changes: the dict is filled as before."""
import copy

import numpy as np

import snn_amd
from snn_amd import ConnectionRule, GraphPosition, WeightRule
from test_connect_rule_host import PAIRS, build_network, closures

SHAPES = {0: (3, 5), 1: (5, 7), 2: (2, 3)}
PLAN = [(0, 1, PAIRS[1]), (2, 1, PAIRS[3]), (1, 0, PAIRS[0]), (2, 0, PAIRS[2])]


def positions(id):
    rows, cols = SHAPES[id]
    return [GraphPosition(id, (r, c)) for r in range(rows) for c in range(cols)]


def connect_by_closure(net, pre, post, rule, weight):
    cond, logic = closures(rule, weight or WeightRule.constant(1.0), SHAPES[post][0] * SHAPES[post][1])(SHAPES[pre][1], SHAPES[post][1])
    net.connect(pre, post, cond, logic)


def twins(plan=PLAN):
    held, by_closure = build_network(), build_network()
    held.hold_connecting_rules = True
    for pre, post, (rule, weight) in plan:
        held.connect(pre, post, rule, weight)
        connect_by_closure(by_closure, pre, post, rule, weight)
    return held, by_closure


def assert_same_answers(held, by_closure):
    assert held.connecting_nodes == by_closure.connecting_nodes
    assert held.connecting_position_to_index == by_closure.connecting_position_to_index
    for pre_id in (0, 1, 2):
        for post_id in (0, 1):
            if pre_id == post_id:
                continue
            for a in positions(pre_id):
                for b in positions(post_id):
                    got, want = held.get_weight(a, b), by_closure.get_weight(a, b)
                    assert isinstance(got, float) and np.float32(got) == np.float32(want), (a.id, a.pos, b.id, b.pos)
    for id in (0, 1):
        for gp in positions(id):
            assert held.get_incoming_connectings_across_lattices(id, gp.pos) == by_closure.get_incoming_connectings_across_lattices(id, gp.pos)
            assert held.get_outgoing_connectings_across_lattices(id, gp.pos) == by_closure.get_outgoing_connectings_across_lattices(id, gp.pos)


def test_record_blocks_answer_as_the_closure_built_network_does():
    held, by_closure = twins()
    assert set(held.connecting_rules) == {(0, 1), (2, 1), (1, 0), (2, 0)} and not held.connecting, "no dict entry per edge"
    assert len(by_closure.connecting) > 0 and not by_closure.connecting_rules
    assert_same_answers(held, by_closure)
    assert set(held.connecting_rules) == {(0, 1), (2, 1), (1, 0), (2, 0)}, "queries must not materialise"
    assert len(held.get_incoming_connectings_across_lattices(1, (2, 2))) > 1, "edges from more than one lattice meet here"
    # the matrix is asked for: the blocks materialise, as lattice.weights does, into the dict the closures fill
    m, want = held.connecting_weights, by_closure.connecting_weights
    assert np.array_equal(np.asarray(m).view(np.uint32), np.asarray(want).view(np.uint32)) and np.asarray(m).any()
    assert not held.connecting_rules and set(held.connecting) == set(by_closure.connecting)
    assert all(np.float32(held.connecting[k]) == np.float32(by_closure.connecting[k]) for k in held.connecting)
    a, b = positions(0)[4], positions(1)[9]
    assert m[a, b] == want[a, b]
    twin_m, twin_want = twins()
    assert np.array_equal(np.asarray(twin_m.get_connecting_weights()), np.asarray(twin_want.get_connecting_weights()))


def test_a_later_connect_replaces_the_block_whichever_form_it_had():
    held, by_closure = twins()
    # a closure on a record block: the record goes, dict entries are written
    rule, weight = PAIRS[0]
    cond, logic = closures(rule, weight, 35)(5, 7)
    for net in (held, by_closure):
        net.connect(0, 1, cond, logic)
    assert (0, 1) not in held.connecting_rules and {k for k in held.connecting} == {k for k in by_closure.connecting if k[0].id == 0 and k[1].id == 1}
    assert_same_answers(held, by_closure)
    # a record on a dict block: its dict entries go, the other blocks' stay
    held.connect(0, 1, *PAIRS[3])
    connect_by_closure(by_closure, 0, 1, *PAIRS[3])
    assert (0, 1) in held.connecting_rules and not held.connecting
    assert_same_answers(held, by_closure)
    # a record on a record block, and a block connected inside a lattice is the lattice's, not the network's
    held.connect(2, 1, *PAIRS[1])
    connect_by_closure(by_closure, 2, 1, *PAIRS[1])
    held.connect(1, 1, *PAIRS[2])
    assert (1, 1) not in held.connecting_rules and held.lattices[1].rule_held
    assert_same_answers(held, by_closure)
    assert np.array_equal(np.asarray(held.connecting_weights).view(np.uint32), np.asarray(by_closure.connecting_weights).view(np.uint32))


def test_deep_copies_carry_the_records():
    held, by_closure = twins()
    twin = copy.deepcopy(held)
    assert twin.hold_connecting_rules and set(twin.connecting_rules) == set(held.connecting_rules) and twin.connecting_rules is not held.connecting_rules
    twin.connect(0, 1, *PAIRS[3])
    assert held.connecting_rules[(0, 1)][0] is not twin.connecting_rules[(0, 1)][0], "the copy's edits stay in the copy"
    assert_same_answers(held, by_closure)
    assert_same_answers(copy.deepcopy(held), by_closure)
    held.clear()
    assert not held.connecting_rules and not held.connecting_nodes


def test_with_the_flag_off_the_dict_is_filled_as_before():
    by_record, by_closure = build_network(), build_network()
    assert by_record.hold_connecting_rules is False and by_record.connecting_rules == {}
    for pre, post, (rule, weight) in PLAN:
        by_record.connect(pre, post, rule, weight)
        connect_by_closure(by_closure, pre, post, rule, weight)
    assert not by_record.connecting_rules
    assert list(by_record.connecting) == list(by_closure.connecting) and len(by_record.connecting) > 0
    assert all(np.float32(by_record.connecting[k]) == np.float32(by_closure.connecting[k]) for k in by_record.connecting)
    assert by_record.connecting_nodes == by_closure.connecting_nodes
    # the GPU classes keep their defaults: dense handles, records into the dict
    assert snn_amd.LatticeNetworkGPU()._sparse is False and snn_amd.LatticeNetworkGPU().network.hold_connecting_rules is False
    sparse = snn_amd.LatticeNetworkGPU(sparse=True)
    assert sparse._sparse and sparse.network.hold_connecting_rules
    assert snn_amd.LatticeGPU(3)._sparse is False and snn_amd.LatticeGPU(3, sparse=True)._sparse
    l = snn_amd.Lattice(4)
    l.populate(snn_amd.IzhikevichNeuron(), 2, 2)
    assert snn_amd.LatticeGPU.from_lattice(l, sparse=True)._sparse and not snn_amd.LatticeGPU.from_lattice(l)._sparse
