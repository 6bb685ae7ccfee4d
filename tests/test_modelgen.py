"""The neuron-description front end (spiking-neural-networks_amd/modelgen.py) on the CPU: it reads the reference's own
DSL file, refuses what it does not implement, and emits the expected HIP for the pieces that carry the arithmetic."""
import numpy as np
import pytest

from snn_amd import modelgen
from snn_amd.examples_dsl import IZH_DSL  # noqa: E402,F401

LIF_NB = """
[neuron]
    type: BasicIntegrateAndFire
    vars: e = 0, v_reset = -75, v_th = -55
    on_spike:
        v = v_reset
    spike_detection: v >= v_th
    on_iteration:
        dv/dt = (v - e) + i
[end]"""          # = /root/reference/build_test/nb_macro/tests/lif.nb (the reference's fixture, restated as data)



def test_parses_the_reference_fixture():
    m = modelgen.parse(LIF_NB)
    assert m.name == "BasicIntegrateAndFire"
    assert m.variables == [("e", 0.0), ("v_reset", -75.0), ("v_th", -55.0)]
    assert m.mandatory == {"current_voltage": 0.0, "dt": 0.1, "c_m": 1.0, "gap_conductance": 10.0}
    assert m.on_iteration == [("diff", "v", ("bin", "+", ("bin", "-", ("var", "v"), ("var", "e")), ("var", "i")))]
    assert m.spike_detection == ("bin", ">=", ("var", "v"), ("var", "v_th"))
    assert m.on_spike == [("assign", "v", "=", ("var", "v_reset"))]
    src = modelgen.hip_source(m)
    assert "const float d_v = (((v - x[0]) + i_in)) * dt;" in src and "v += d_v;" in src
    assert "const bool spiking = (v >= x[2]);" in src and "v = x[1];" in src


def test_mandatory_overrides_precedence_and_order_of_application():
    m = modelgen.parse(IZH_DSL)
    assert m.mandatory["c_m"] == 100.0 and m.mandatory["current_voltage"] == -65.0
    assert [n for n, _ in m.variables] == ["a", "b", "c", "d", "w", "v_th", "tau_m"]
    src = modelgen.hip_source(m)
    # left-to-right, one operation per node; both derivatives are formed before either variable moves
    assert "((((((0.03999999910593033f * v) * v) + (5.0f * v)) + 140.0f) - x[4]) + i_in) + " in src
    assert "(0.5f * expf_glibc(((v - x[5]) / 20.0f)))) / c_m)" in src
    i_dv, i_dw, i_apply = src.index("const float d_v"), src.index("const float d_x4"), src.index("v += d_v;")
    assert i_dv < i_dw < i_apply < src.index("x[4] += d_x4;")
    assert "x[4] += x[3];" in src                  # on_spike: w += d


@pytest.mark.parametrize("text,needle", [
    (LIF_NB.replace("dv/dt = (v - e) + i", "dv/dt = (v - e) ^ true"), "needs a number"),
    (LIF_NB.replace("dv/dt = (v - e) + i", "dv/dt = log(v)"), "log"),
    (LIF_NB.replace("dv/dt = (v - e) + i", "dv/dt = isnan(v)"), "needs a number"),
    (LIF_NB.replace("dv/dt = (v - e) + i", "dv/dt = min(v)"), "argument"),
    (LIF_NB.replace("spike_detection: v >= v_th", "spike_detection: continuous()").replace(", v_th = -55", ""),
     "continuous() compares with v_th"),
    (LIF_NB.replace("spike_detection: v >= v_th", "spike_detection: continuous()").replace("vars: e = 0", "vars: last_voltage = 0, e = 0"),
     "keeps its own 'last_voltage'"),
    (LIF_NB.replace("vars: e = 0", "vars: flag = true, e = 0").replace("(v - e) + i", "(v - e) + flag"), "needs a number"),
    (LIF_NB.replace("spike_detection: v >= v_th", "spike_detection: v"), "spike_detection needs a bool"),
    (LIF_NB.replace("vars: e = 0", "vars: flag = true, e = 0").replace("v = v_reset", "flag = 3"), "assignment to flag"),
    (LIF_NB.replace("vars: e = 0", "vars: flag = true, e = 0").replace("v = v_reset", "flag += true"), "on the bool variable"),
    (LIF_NB.replace("vars: e = 0", "vars: dt = true, e = 0"), "is a number"),
    (LIF_NB.replace("dv/dt = (v - e) + i", "dv/dt = (v - q) + i"), "unknown variable"),
    (LIF_NB.replace("[neuron]", "[synapse]"), "text outside a block"),
    (LIF_NB + "\n" + LIF_NB, "exactly one [neuron]"),
    (LIF_NB.replace("on_iteration:", "ion_channels: k = K\n    on_iteration:"), "unknown ion channel type"),
    (LIF_NB.replace("dv/dt = (v - e) + i", "k.update_current(v)\n        dv/dt = (v - e) + i"), "cannot call"),
    (LIF_NB.replace("v = v_reset", "dt = 1"), "cannot assign"),
])
def test_unsupported_descriptions_are_refused_with_a_reason(text, needle):
    with pytest.raises(modelgen.ModelError) as e:
        modelgen.parse(text)
    assert needle in str(e.value)


def test_interpreter_reproduces_the_reference_hand_expansion():
    """build_test/nb_macro/tests/lif_reference.rs (the struct basic_lif.rs compares the generated code with):
    dv = ((V - e) + I) * dt; V += dv; spike = V >= v_th; if spike V = v_reset -- 1000 iterations for each input of
    basic_lif.rs:22."""
    import modelgen_ref
    f32 = np.float32
    m = modelgen.parse(LIF_NB)
    step = modelgen_ref.make_step(m)
    currents = np.array([-50., -40., -30., -20., -10., 0., 10., 20., 30., 40., 50.], f32)
    n = currents.size
    st = {"current_voltage": np.zeros(n, f32), "dt": np.full(n, 0.1, f32), "c_m": np.ones(n, f32),
          "gap_conductance": np.full(n, 10.0, f32), "e": np.zeros(n, f32), "v_reset": np.full(n, -75.0, f32),
          "v_th": np.full(n, -55.0, f32)}
    v = np.zeros(n, f32)
    old = np.seterr(over="ignore", invalid="ignore")       # the leak is positive: voltages run away to -inf
    for _ in range(1000):
        spike = step(st, currents)
        dv = (((v - f32(0.0)).astype(f32) + currents).astype(f32) * f32(0.1)).astype(f32)
        v = (v + dv).astype(f32)
        ref_spike = v >= f32(-55.0)
        v = np.where(ref_spike, f32(-75.0), v).astype(f32)
        assert np.array_equal(spike, ref_spike) and np.array_equal(st["current_voltage"].view(np.uint32), v.view(np.uint32))
    np.seterr(**old)


def test_oracle_stack_program_equals_the_numpy_interpreter():
    """Two independent evaluators of the same description: the C oracle's stack program (snn_oracle.c::step_custom,
    compiled by modelgen_ref.compile_program) and the numpy interpreter inside numpy_ref.run_lattice."""
    import modelgen_ref
    import numpy_ref as nr
    import oracle_binding as ob
    import parity
    m = modelgen.parse(IZH_DSL)
    net = parity.make_oracle(parity.Layout([(0, 5, 6)]), model=ob.CUSTOM)
    modelgen_ref.attach(net, m)
    n = net.n_neurons
    net["current_voltage"] = ob.uniform_array(3, n, -65.0, 30.0)
    net["gap_conductance"] = 4.0
    net.fill_graph(4, 0.5, 1.5)
    st = {k: net[k].copy() for k in ("current_voltage", "dt", "c_m", "gap_conductance")}
    for k, (name, _) in enumerate(m.variables):
        st[name] = net["custom_vars"][k].copy()
    vh, sh, lft = nr.run_lattice(modelgen_ref.make_step(m), st, st["gap_conductance"].copy(), net["weights"].copy(),
                                 net["connections"].copy(), 900)
    net.run(900, voltage_history=True, spike_history=True)
    assert sh.sum() > 5
    assert np.array_equal(sh, net.spike_history)
    assert np.array_equal(vh.view(np.uint32), net.voltage_history.view(np.uint32))
    assert np.array_equal(st["w"].view(np.uint32), net["custom_vars"][4].view(np.uint32))


IF_DSL = """
[neuron]
    type: ElseIfNestedBasicIntegrateAndFire
    vars: e = 0, v_reset = -75, v_th = -55, flag = 0
    on_spike:
        v = v_reset
    spike_detection: v >= v_th
    on_iteration:
        dv/dt = (v - e) + i
        [if] i < 0 [then]
            flag = 1
        [elseif] i > 20 [then]
            [if] i >= 40 [then]
                flag = 2
            [else]
                flag = 3
            [end]
        [else]
            flag = 4
        [end]
[end]"""          # the last model of build_test/nb_macro/tests/if_statements.rs (restated as data)

CURRENTS = np.array([-50., -40., -30., -20., -10., 0., 10., 20., 30., 40., 50.], np.float32)      # if_statements.rs:127
EXPECTED_FLAG = np.where(CURRENTS < 0, 1.0, np.where(CURRENTS > 20, np.where(CURRENTS >= 40, 2.0, 3.0), 4.0)).astype(np.float32)


def lif_reference_trace(steps):
    """ReferenceIntegrateAndFire (build_test/nb_macro/tests/lif_reference.rs) for the eleven input currents"""
    f32 = np.float32
    v = np.zeros(CURRENTS.size, f32)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(steps):
            dv = (((v - f32(0.0)).astype(f32) + CURRENTS).astype(f32) * f32(0.1)).astype(f32)
            v = (v + dv).astype(f32)
            v = np.where(v >= f32(-55.0), f32(-75.0), v).astype(f32)
            out.append(v.copy())
    return np.array(out)


def test_if_statements_known_answers_on_both_cpu_evaluators():
    """if_statements.rs: the branches taken depend on the input current only; voltages stay those of the plain LIF.
    Checked on the numpy interpreter and on the C oracle's stack program (jumps)."""
    import modelgen_ref
    import oracle_binding as ob
    import parity
    f32 = np.float32
    m = modelgen.parse(IF_DSL)
    assert m.on_iteration[1][0] == "if" and len(m.on_iteration[1][1]) == 2 and m.on_iteration[1][2] is not None
    src = modelgen.hip_source(m)
    assert "} else if ((i_in > 20.0f)) {" in src and "if ((i_in >= 40.0f)) {" in src
    n = CURRENTS.size
    ref = lif_reference_trace(300)
    # numpy interpreter
    step = modelgen_ref.make_step(m)
    st = {"current_voltage": np.zeros(n, f32), "dt": np.full(n, 0.1, f32), "c_m": np.ones(n, f32),
          "gap_conductance": np.full(n, 10.0, f32), "e": np.zeros(n, f32), "v_reset": np.full(n, -75.0, f32),
          "v_th": np.full(n, -55.0, f32), "flag": np.zeros(n, f32)}
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(300):
            step(st, CURRENTS)
            assert np.array_equal(st["flag"], EXPECTED_FLAG)
            assert np.array_equal(st["current_voltage"].view(np.uint32), ref[t].view(np.uint32))
    # C oracle: each neuron gets its current from a never-firing cell (v_resting enters the sum as it is)
    lay = parity.Layout([(1, 1, n)], [(0, 1, n)])
    net = parity.make_oracle(lay, model=ob.CUSTOM, st_kind=ob.ST_RATE)
    modelgen_ref.attach(net, m)
    net["st_v_resting"] = CURRENTS
    net["connections"][n + np.arange(n), np.arange(n)] = 1
    net["weights"][n + np.arange(n), np.arange(n)] = 1.0
    net.run(300, voltage_history=True)
    assert np.array_equal(net["custom_vars"][3], EXPECTED_FLAG)
    assert np.array_equal(net.voltage_history.view(np.uint32), ref.view(np.uint32))


BOOL_DSL = """
[neuron]
    type: BoolIntegrateAndFire
    vars: e = 0, v_reset = -75, v_th = -55, flag = false, out = 0, seen = false
    on_spike:
        v = v_reset
        seen = true
    spike_detection: v >= v_th
    on_iteration:
        [if] flag [then]
            out = 1
        [else]
            out = 2
        [end]
        [if] !flag && seen == true [then]
            out = out + 10
        [end]

        dv/dt = (v - e) + i
[end]"""          # build_test/nb_macro/tests/bool_vars.rs:10-26 plus a bool written by on_spike and read through ! && ==


def bool_expected_out(flag, steps):
    """out after `steps` iterations: 1 / 2 by flag (bool_vars.rs:56-60), +10 once the neuron has fired and flag is false
    (the plain LIF above threshold fires on its first step for every current of CURRENTS >= -50: v starts at 0)"""
    fired_before = steps > 1
    return np.where(flag, 1.0, np.where(fired_before, 12.0, 2.0)).astype(np.float32)


def test_bool_variables_known_answers_on_both_cpu_evaluators():
    import modelgen_ref
    import oracle_binding as ob
    import parity
    f32 = np.float32
    m = modelgen.parse(BOOL_DSL)
    assert m.bools == {"flag", "seen"} and dict(m.variables)["flag"] == 0.0
    src = modelgen.hip_source(m)
    assert "if ((x[3] != 0.0f)) {" in src and "x[5] = true ? 1.0f : 0.0f;" in src
    currents = np.concatenate([CURRENTS, CURRENTS])
    flag = np.concatenate([np.zeros(CURRENTS.size, bool), np.ones(CURRENTS.size, bool)])
    n = currents.size
    ref = np.concatenate([lif_reference_trace(300)] * 2, axis=1)
    step = modelgen_ref.make_step(m)
    st = {"current_voltage": np.zeros(n, f32), "dt": np.full(n, 0.1, f32), "c_m": np.ones(n, f32),
          "gap_conductance": np.full(n, 10.0, f32)}
    for name, default in m.variables:
        st[name] = np.full(n, default, f32)
    st["flag"] = flag.astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(300):
            step(st, currents)
            assert np.array_equal(st["out"], bool_expected_out(flag, t + 1)), t
            assert np.array_equal(st["current_voltage"].view(np.uint32), ref[t].view(np.uint32))
    assert st["seen"].all()
    lay = parity.Layout([(1, 1, n)], [(0, 1, n)])
    net = parity.make_oracle(lay, model=ob.CUSTOM, st_kind=ob.ST_RATE)
    modelgen_ref.attach(net, m)
    names = [name for name, _ in m.variables]
    net["custom_vars"][names.index("flag")] = flag.astype(f32)
    net["st_v_resting"] = currents
    net["connections"][n + np.arange(n), np.arange(n)] = 1
    net["weights"][n + np.arange(n), np.arange(n)] = 1.0
    net.run(300, voltage_history=True)
    assert np.array_equal(net["custom_vars"][names.index("out")], bool_expected_out(flag, 300))
    assert np.array_equal(net["custom_vars"][names.index("seen")], np.ones(n, f32))
    assert np.array_equal(net.voltage_history.view(np.uint32), ref.view(np.uint32))


def test_if_statement_errors():
    for text, needle in [(IF_DSL.replace("            [end]\n        [else]", "        [else]"), "[end]"),
                         (IF_DSL.replace("flag = 1", "dflag/dt = 1"), "top level"),
                         (IF_DSL.replace("[elseif] i > 20 [then]", "[elseif] i > 20"), "cannot read statement")]:
        with pytest.raises(modelgen.ModelError) as e:
            modelgen.parse(text)
        assert needle in str(e.value), (needle, str(e.value))


@pytest.mark.parametrize("seed", range(12))
def test_random_descriptions_cpu_evaluators_agree(seed):
    """Property test of the two CPU evaluators the device is held to: random expressions (every operator and function,
    if / else, earlier results as operands) through the numpy interpreter and through the C oracle's stack program."""
    import modelgen_ref
    import oracle_binding as ob
    import parity
    import random_descriptions
    m = modelgen.parse(random_descriptions.description(seed))
    n = 48
    x = ob.uniform_array(100 + seed, n, -4.0, 4.0)
    params = {"a": ob.uniform_array(200 + seed, n, -2.0, 2.0), "b": ob.uniform_array(300 + seed, n, -2.0, 2.0),
              "c": ob.uniform_array(400 + seed, n, 0.1, 3.0)}
    names = [name for name, _ in m.variables]
    step = modelgen_ref.make_step(m)
    st = {"current_voltage": np.zeros(n, np.float32), "dt": np.full(n, 0.1, np.float32), "c_m": np.ones(n, np.float32),
          "gap_conductance": np.full(n, 10.0, np.float32)}
    for name, default in m.variables:
        st[name] = np.full(n, default, np.float32)
    st.update({k: v.copy() for k, v in params.items()})
    with np.errstate(all="ignore"):
        step(st, x)
        step(st, x)
    lay = parity.Layout([(1, 1, n)], [(0, 1, n)])
    net = parity.make_oracle(lay, model=ob.CUSTOM, st_kind=ob.ST_RATE)
    modelgen_ref.attach(net, m)
    for k, v in params.items():
        net["custom_vars"][names.index(k)] = v
    net["st_v_resting"] = x
    net["connections"][n + np.arange(n), np.arange(n)] = 1
    net["weights"][n + np.arange(n), np.arange(n)] = 1.0
    net.run(2)
    finite = 0
    for k, name in enumerate(names):
        assert np.array_equal(parity.bits(net["custom_vars"][k]), parity.bits(st[name])), (seed, name)
        finite += int(np.isfinite(st[name]).sum())
    assert finite > 0.7 * n * len(names)


def test_description_file_reader(tmp_path, monkeypatch):
    """neuron_builder_from_file (the reference's macro of that name, basic_lif_from_file.rs:9): the file's text goes
    through neuron_builder; here with the compile step stubbed out (hipcc runs in the GPU suite)."""
    import snn_amd
    from snn_amd import _lib
    path = tmp_path / "lif.nb"
    path.write_text(LIF_NB)
    monkeypatch.setattr(_lib, "build_custom", lambda model, force=False: "/nonexistent/" + model.name + ".so")
    Neuron, LatticeCls, LatticeGPUCls = snn_amd.neuron_builder_from_file(str(path))
    assert Neuron.__name__ == "BasicIntegrateAndFire" and Neuron().v_reset == -75.0 and Neuron.model == snn_amd.CUSTOM
    assert LatticeCls.neuron_type is Neuron and LatticeGPUCls.lattice_type is LatticeCls
    assert Neuron.lib_path.endswith("BasicIntegrateAndFire.so")
    with pytest.raises(modelgen.ModelError):
        path.write_text(LIF_NB.replace("[end]", ""))
        snn_amd.neuron_builder_from_file(str(path))
