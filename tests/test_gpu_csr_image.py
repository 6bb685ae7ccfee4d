"""The step image of a sparse handle (csrc/snn_kernels_csr.hpp "STEP IMAGE", k_step_csr_img): 16-byte records of two entries and
the slices' presynaptic windows staged in LDS.  Bit for bit the oracle -- and the plain one-launch step -- on: the structure of
BASELINE configs[4] (every slice staged), unstructured graphs (no slice staged: plain codes through the records), graphs that mix
both, ragged and empty rows, rows far longer than the record ring, chunk crossings, Rate cells that have never fired (the view's
second word), and a handle whose weights change in between (plasticity on, then off: the records are rebuilt).
Directed graphs (from_rows) put the window's edges where a random graph never does: a slice whose rows read exactly the 1024 words
of a window -- as the last wavefront of its workgroup --, one source more, sixteen pieces with gaps, trimmed pieces; 512 cells up to
the last cell of the array (its view words at window words 1022 / 1023), 513 cells, the neuron | cell boundary inside a run of
consecutive codes; row lengths around the ring of four records with odd widths, empty slices in the middle and at the end; and all
eight built-in models.  Every directed test restates the host's greedy cut in numpy (greedy_cut) and asserts its own construction
from it before a GPU is touched."""
import numpy as np
import pytest

import oracle_binding as ob
import parity
from test_gpu_csr import c5_structure

pytestmark = pytest.mark.gpu


def run_both(snn, net, steps, expect_staged=None, histories=True):
    """the same network with and without the image, against the oracle; returns the image handle's statistics"""
    ref = None
    stats = {}
    for image in (1, 0):
        dn = parity.device_from_oracle(snn, net, csr=True)
        dn.set_option("csr_image", image)
        if histories:
            dn.set_history(voltage=True, spikes=True)
        dn.run(steps // 2)
        dn.run(steps - steps // 2)
        st = parity.pull_state(dn, net)
        hist = [(parity.bits(dn.voltage_history(i)), dn.spike_history(i)) for i, _, _ in net.layout.lattices] if histories else []
        if image:
            stats = {k: dn.stat(k) for k in ("steps_sparse_image", "steps_sparse_one_launch", "image_staged_slices")}
            ref = (st, hist)
        else:
            assert dn.stat("steps_sparse_image") == 0
            for k in ref[0]:
                assert np.array_equal(parity.bits(ref[0][k]), parity.bits(st[k])), k
            for (va, sa), (vb, sb) in zip(ref[1], hist):
                assert np.array_equal(va, vb) and np.array_equal(sa, sb)
        dn.close()
    onet = net
    onet.run(steps, voltage_history=histories, spike_history=histories)
    parity.assert_state_equal(onet, ref[0])
    rng = net.layout.ranges()
    for (i, _, _), (v, s) in zip(net.layout.lattices, ref[1]):
        first, count, _ = rng[i]
        assert np.array_equal(s, onet.spike_history[:, first:first + count])
        assert np.array_equal(v, parity.bits(onet.voltage_history[:, first:first + count]))
    assert stats["steps_sparse_image"] == steps == stats["steps_sparse_one_launch"]
    if expect_staged is not None:
        assert stats["image_staged_slices"] == expect_staged, stats
    return stats


def test_the_structure_of_configs4_is_staged_slice_by_slice(snn):
    net = c5_structure(24)                               # 4 x 576 neurons + as many Poisson cells; 14 entries per interior row
    st = run_both(snn, net, 60, expect_staged=(4 * 576 + 63) // 64)
    assert st["image_staged_slices"] == 36


def sparse(layout, st_layout, seed, st_kind=ob.ST_RATE, density=0.04, band=None, long_rows=()):
    """a graph drawn at random; band = neurons only read sources within that distance (a structured graph: stageable)"""
    net = parity.make_oracle(parity.Layout(layout, st_layout), st_kind=st_kind)
    nn, nc = net.n_neurons, net.n_cells
    rng = np.random.default_rng(seed)
    net["current_voltage"] = ob.uniform_array(seed, nn, -65.0, 30.0)
    net["gap_conductance"] = 8.0 + 4.0 * rng.random(nn).astype(np.float32)          # per-neuron conductances
    net.fill_graph(seed + 1, 0.2, 1.2, with_diagonal=True)
    conn = rng.random(net["connections"].shape) < density
    if band is not None:
        p, q = np.meshgrid(np.arange(net.n_tot), np.arange(nn), indexing="ij")
        conn &= (np.abs(p - q) <= band) | (p >= nn)
    for q in long_rows:
        conn[:, q] = rng.random(net.n_tot) < 0.6
    net["connections"][...] = conn
    net["weights"][...] *= net["connections"]
    if nc:
        if st_kind == ob.ST_RATE:
            net["st_rate"] = np.where(np.arange(nc) % 3 == 0, 0.0, 0.4 + 0.2 * (np.arange(nc) % 5)).astype(np.float32)   # a third never fires
        else:
            net["st_chance_of_firing"] = 0.03
            net["st_seed"] = np.arange(11, 11 + nc, dtype=np.uint32)
    return net


def test_an_unstructured_graph_goes_through_the_records_with_plain_codes(snn):
    net = sparse([(0, 30, 30), (3, 17, 19)], [(5, 6, 6)], seed=21, density=0.05)
    st = run_both(snn, net, 80)
    assert st["image_staged_slices"] == 0                                # (3 of 64 sources per piece: sixteen pieces never cover a slice)


def test_staged_and_unstaged_slices_in_one_launch_with_ragged_and_long_rows(snn):
    # banded rows (stageable) + a few rows that read 60 % of everything (their slices are not), an empty row, rows past a ragged end
    # (a window holds 1024 words: a network must be larger than that for a slice's sources not to fit)
    net = sparse([(0, 40, 40), (2, 9, 11)], [(4, 5, 7)], seed=33, density=0.5, band=6, long_rows=(3, 300, 1501))
    net["connections"][:, 77] = 0
    net["weights"][:, 77] = 0
    st = run_both(snn, net, 40)
    n_slices = (net.n_neurons + 63) // 64
    assert 0 < st["image_staged_slices"] < n_slices
    assert net["connections"].sum(axis=0).max() > 500                   # far past the ring of four records


@pytest.mark.parametrize("st_kind", [ob.ST_RATE, ob.ST_POISSON])
def test_cells_through_the_window_fired_and_never_fired(snn, st_kind):
    net = sparse([(0, 16, 16)], [(1, 8, 8)], seed=5, st_kind=st_kind, density=0.6, band=3)
    net["connections"][net.n_neurons:, :] = np.random.default_rng(1).random((net.n_cells, net.n_neurons)) < 0.1
    net["weights"][net.n_neurons:, :] = net["connections"][net.n_neurons:, :] * np.float32(1.5)
    run_both(snn, net, 90)


def test_weights_that_change_in_between_rebuild_the_records(snn):
    net = sparse([(0, 14, 14)], [(1, 3, 3)], seed=8, density=0.7, band=4)
    dn = parity.device_from_oracle(snn, net, csr=True)
    dn.run(20)
    assert dn.stat("steps_sparse_image") == 20
    dn.set_plasticity(0, do_plasticity=True)             # STDP on: the plain kernels step, weights move
    net["do_plasticity"] = 1
    dn.run(40)
    assert dn.stat("steps_sparse_image") == 20
    dn.set_plasticity(0, do_plasticity=False)            # off again: the image comes back with the NEW weights
    net["do_plasticity"] = 0
    dn.run(30)
    assert dn.stat("steps_sparse_image") == 50
    net.run(20)
    net["do_plasticity"] = 1
    net.run(40)
    net["do_plasticity"] = 0
    net.run(30)
    assert not np.array_equal(net["weights"], sparse([(0, 14, 14)], [(1, 3, 3)], seed=8, density=0.7, band=4)["weights"])
    parity.assert_state_equal(net, parity.pull_state(dn, net))
    parity.assert_graph_equal(net, dn)
    # a checkpoint restore puts old weights back: again a rebuild
    dn.checkpoint()
    dn.set_plasticity(0, do_plasticity=True)
    dn.run(10)
    dn.set_plasticity(0, do_plasticity=False)
    dn.restore_checkpoint()
    dn.run(15)
    net.run(15)
    parity.assert_state_equal(net, parity.pull_state(dn, net))
    dn.close()


# ---- directed graphs: the window's and the record ring's edges ---------------------------------------------------------------------
def greedy_cut(net):
    """the host's cut of every slice's sources into window pieces (csrc/snn_step_image_plan.hpp), restated: per slice
    (pieces needed, largest window word an entry reads) -- a piece starts at the smallest source not yet covered and covers what
    follows within 64 words (a neuron is one word, a cell two) without leaving the neurons resp. the cells.  A slice is staged
    when it needs 1 .. 16 pieces."""
    nn, n_tot, conn = net.n_neurons, net.n_tot, net["connections"]
    out = []
    for s0 in range(0, nn, 64):
        codes = np.flatnonzero(conn[:, s0:s0 + 64].any(axis=1))
        pieces, top, i = 0, -1, 0
        while i < len(codes):
            cell = codes[i] >= nn
            end = min(codes[i] + (32 if cell else 64), n_tot if cell else nn)
            j = int(np.searchsorted(codes, end))
            top = pieces * 64 + int(codes[j - 1] - codes[i]) * (2 if cell else 1)
            pieces, i = pieces + 1, j
        out.append((pieces, top))
    return out


def staged_slices(net):
    return sum(1 for pieces, _ in greedy_cut(net) if 1 <= pieces <= 16)


def from_rows(layout, st_layout, rows, seed, st_kind=ob.ST_RATE, band=3, **kw):
    """rows = {slice: 64 sequences of presynaptic indices (neuron p, cell nn + c)}; the rows of every other slice read the neurons
    within `band` of themselves (two pieces: staged).  Distinct voltages, per-neuron conductances, random weights."""
    net = parity.make_oracle(parity.Layout(layout, st_layout), st_kind=st_kind if st_layout else ob.ST_NONE, **kw)
    nn = net.n_neurons
    rng = np.random.default_rng(seed)
    net["current_voltage"] = ob.uniform_array(seed, nn, -65.0, 30.0)
    assert len(np.unique(net["current_voltage"])) == nn                  # a misplaced window word changes a sum
    net["gap_conductance"] = 8.0 + 4.0 * rng.random(nn).astype(np.float32)
    net.fill_graph(seed + 1, 0.2, 1.2, with_diagonal=True)
    conn = np.zeros(net["connections"].shape, bool)
    for q in range(nn):
        if q // 64 in rows:
            src = rows[q // 64][q % 64] if q % 64 < len(rows[q // 64]) else ()
            conn[np.asarray(src, dtype=np.int64), q] = True
        else:
            conn[max(0, q - band):min(nn, q + band + 1), q] = True
    net["connections"][...] = conn
    net["weights"][...] *= net["connections"]
    return net


def test_a_window_exactly_full_in_the_last_wavefront_of_its_workgroup_and_one_source_more(snn):
    # slice 3 = the fourth wavefront of workgroup 0: its 64 rows read 16 neurons each, together exactly the 1024 neurons from 37 on
    # (every window word by exactly one row; the last at word 1023, the last word of the workgroup's LDS); slice 7: 1025 neurons, not
    # staged, in the same launch; slice 11: 1024 neurons in sixteen full pieces with gaps of 6 between them; slice 15: sixteen
    # pieces trimmed to 40, 41, ... words
    full = np.arange(37, 37 + 1024)
    more = np.arange(301, 301 + 1025)
    gaps = np.concatenate([5 + 70 * u + np.arange(64) for u in range(16)])
    trimmed = np.concatenate([[9 + 90 * u, 9 + 90 * u + 11, 9 + 90 * u + 25, 9 + 90 * u + 39 + u] for u in range(16)])
    rows = {3: np.split(full, 64), 7: np.split(more[:1024], 64)[:63] + [more[1008:]], 11: np.split(gaps, 64), 15: np.split(trimmed, 64)}
    net = from_rows([(0, 40, 40)], [], rows, seed=41)
    cut = greedy_cut(net)
    assert len(cut) == 25 and 37 % 64 and cut[3] == (16, 1023) and cut[7][0] == 17 and cut[11] == (16, 1023) and cut[15] == (16, 15 * 64 + 39 + 15)
    assert all(c[0] == 2 for i, c in enumerate(cut) if i not in rows)                # the banded rest
    assert (net["connections"][:, 192:256].sum(axis=1) <= 1).all() and net["connections"][:, 192:256].sum() == 1024
    run_both(snn, net, 30, expect_staged=24)


@pytest.mark.parametrize("last_cell_fires", [False, True])
@pytest.mark.parametrize("st_kind", [ob.ST_RATE, ob.ST_POISSON])
def test_cells_up_to_the_last_cell_at_the_windows_last_words(snn, st_kind, last_cell_fires):
    # 256 neurons + 544 cells.  Slice 3 (the last wavefront of its workgroup): 512 consecutive cells up to the LAST cell of the
    # array, sixteen pieces of 32 cells, the last cell's two view words at window words 1022 / 1023; slice 2: 513 cells, not
    # staged; slice 1: neurons nn - 3 .. nn - 1 and cells 0 .. 2 -- consecutive codes of two kinds, two pieces
    nn, nc = 256, 544
    cells = nn + np.arange(nc)
    rows = {3: np.split(cells[nc - 512:], 64), 2: np.split(cells[nc - 513:nc - 1], 64)[:63] + [cells[nc - 9:]],
            1: [np.arange(nn - 3, nn + 3)[(i % 3):] for i in range(64)]}
    net = from_rows([(0, 16, 16)], [(1, 17, 32)], rows, seed=44, st_kind=st_kind)
    net["connections"][nn:nn + 40:3, :64] = 1                                        # (slice 0: its band and a few cells)
    net["weights"][nn:, :] = net["connections"][nn:, :] * np.float32(1.5)
    # never-fired cells (the view's second word is set) and fired ones at both ends of the pieces: piece u holds cells
    # 32 + 32 u .. 63 + 32 u; its first cell never fires when u is even, its last when u is odd -- but for the LAST cell, set below
    c = np.arange(nc)
    u = (c - 32) // 32
    silent = ((c % 32 == 0) & (u % 2 == 0)) | ((c % 32 == 31) & (u % 2 == 1)) | (c % 7 == 3)
    silent[nc - 1] = not last_cell_fires
    if st_kind == ob.ST_RATE:
        net["st_rate"] = np.where(silent, 0.0, 0.4 + 0.2 * (c % 5)).astype(np.float32)
    else:
        net["st_chance_of_firing"] = np.where(silent, 0.0, 0.2).astype(np.float32)
        net["st_seed"] = np.arange(11, 11 + nc, dtype=np.uint32)
    cut = greedy_cut(net)
    assert cut[3] == (16, 1022) and cut[2][0] == 17 and cut[1] == (2, 64 + 4) and 1 <= cut[0][0] <= 16
    assert net["connections"][nn + nc - 1, 192:256].sum() == 1
    run_both(snn, net, 40, expect_staged=3)
    fired = net["st_last_firing_time"] >= 0                                         # (run_both has run the oracle)
    assert fired[nc - 1] == last_cell_fires and not fired[silent].any() and fired[~silent].all()


RING_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17)       # around the ring of 4 records = 8 entries, summed four at a time


def canonical_sum(net, q, flush=True):
    """row q's electrical input of the first step in binary32, as the kernels sum it: ascending, a partial per 256-index chunk
    (flush=False: one running sum -- what a misplaced flush would give)"""
    v, g, w = net["current_voltage"], net["gap_conductance"], net["weights"]
    total, part, chunk = np.float32(0), np.float32(0), None
    for p in np.flatnonzero(net["connections"][:, q]):
        if flush and chunk is not None and p // 256 != chunk:
            total, part = np.float32(total + part), np.float32(0)
        chunk = p // 256
        part = np.float32(part + np.float32(np.float32(g[q] * np.float32(v[p] - v[q])) * w[p, q]))
    return np.float32(total + part)


def test_row_lengths_around_the_record_ring_odd_widths_and_empty_slices(snn):
    # 33 x 35 = 1155 neurons: 19 slices, the last one of 3 rows.  Slice 2: row lengths RING_LENGTHS repeated, width 17 (odd: half
    # a record of padding), every row's sources across a 256-index chunk boundary; slice 4: the same lengths, sources 70 apart
    # (one piece each: not staged -- the ring of the plain codes); slices of width 8, 9 and 1; slice 12 empty in the middle; the
    # LAST slice empty (its lanes read the records' slack)
    nn = 33 * 35
    assert nn % 64 and nn % 256
    lengths = [RING_LENGTHS[i % len(RING_LENGTHS)] for i in range(64)]
    across = [256 * (1 + i % 4) - n // 2 + np.arange(n) for i, n in enumerate(lengths)]
    apart = [3 + i % 5 + 70 * np.arange(n) for i, n in enumerate(lengths)]
    rows = {2: across, 4: apart, 6: [200 + np.arange(8 if i % 3 else 5) for i in range(64)], 8: [250 + np.arange(9 if i == 40 else i % 9) for i in range(64)],
            10: [[700 + i] if i % 2 else [] for i in range(64)], 12: [], 18: []}
    net = from_rows([(0, 33, 35)], [], rows, seed=47)
    width = net["connections"].reshape(net.n_tot, -1)[:, :1152].reshape(net.n_tot, 18, 64).sum(axis=0).max(axis=1)
    assert [int(width[i]) for i in (2, 4, 6, 8, 10, 12)] == [17, 17, 8, 9, 1, 0] and net["connections"][:, 1152:].sum() == 0
    assert sorted(set(net["connections"][:, 128:192].sum(axis=0))) == sorted(RING_LENGTHS)
    cut = greedy_cut(net)
    assert len(cut) == 19 and cut[2][0] == 4 and cut[4][0] == 17 and cut[12] == (0, -1) and cut[18] == (0, -1)
    # the chunk flush is part of what is compared: without it (or with it in another place) these rows' sums are other floats
    crossing = [q for q in range(128, 192) if lengths[q - 128] >= 2]
    assert sum(canonical_sum(net, q) != canonical_sum(net, q, flush=False) for q in crossing) >= len(crossing) // 4
    run_both(snn, net, 30, expect_staged=16)


MODEL_STATE = {            # voltages and parameters as tests/test_gpu_models.py sets them for each model
    ob.IZHIKEVICH: dict(v=(-65.0, 30.0)),
    ob.LIF: dict(v=(-80.0, -50.0), tref=(0.5, 2.0)),
    ob.HH: dict(v=(-70.0, -60.0)),
    ob.QIF: dict(v=(-75.0, -56.0), tref=(0.3, 1.5), tau_m=10.0),
    ob.SIMPLE_LIF: dict(v=(-75.0, -56.0), slif_g=0.5, slif_e=-76.0),
    ob.ADAPTIVE_LIF: dict(v=(-75.0, -56.0), tref=(0.3, 1.5), adp_beta=(1.0, 4.0), adp_alpha=(3.0, 8.0), leak_constant=1.0, v_reset=-73.0),
    ob.ADAPTIVE_EXP_LIF: dict(v=(-75.0, -56.0), tref=(0.3, 1.5), adp_beta=(1.0, 4.0), adp_alpha=(3.0, 8.0), leak_constant=1.0, v_reset=-73.0,
                              slope_factor=(0.5, 3.0)),
    ob.LEAKY_IZHIKEVICH: dict(v=(-65.0, 30.0), w_value=(0.0, 1.0), e_l=(-70.0, -60.0)),
}


@pytest.mark.parametrize("model", sorted(MODEL_STATE), ids=["izhikevich", "lif", "hodgkin_huxley", "qif", "simple_lif", "adaptive_lif", "adaptive_exp_lif",
                                                            "leaky_izhikevich"])
def test_every_models_image_kernel_steps_staged_and_unstaged_slices(snn, model):
    # 36 x 36 neurons + 12 Rate cells: banded slices (staged), slice 5 with sources 70 apart (not staged), slice 9 reads the cells
    nn = 36 * 36
    rows = {5: [2 + i % 7 + 70 * np.arange(18) for i in range(64)],
            9: [np.concatenate([576 + i + np.arange(-2, 3), nn + np.arange(i % 4, 12, 3)]) for i in range(64)]}
    net = from_rows([(0, 36, 36)], [(1, 1, 12)], rows, seed=53 + model, model=model)
    state = MODEL_STATE[model]
    net["current_voltage"] = ob.uniform_array(60 + model, nn, *state["v"])
    for i, (name, value) in enumerate(sorted(state.items())):
        if name != "v":
            net[name] = ob.uniform_array(70 + i, nn, *value) if isinstance(value, tuple) else value
    net["weights"][nn:, :] = net["connections"][nn:, :] * np.float32(1.5)
    net["st_rate"] = np.where(np.arange(12) % 3 == 0, 0.0, 0.4 + 0.2 * (np.arange(12) % 5)).astype(np.float32)      # a third never fires
    cut = greedy_cut(net)
    assert len(cut) == 21 and cut[5][0] == 18 and 1 <= cut[9][0] <= 16
    st = run_both(snn, net, 30, expect_staged=20)
    assert st["steps_sparse_image"] == 30                                # this model's k_step_csr_img has stepped
    assert np.isfinite(net["current_voltage"]).all()
