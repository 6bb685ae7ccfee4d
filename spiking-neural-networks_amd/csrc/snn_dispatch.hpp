// Run-time values to template arguments (host only): each helper hands the value as a type (int_c / bool_c) to a generic
// lambda, which names the kernel it launches -- snn_network_step.hpp.  And the ONE place that says which neuron models the
// model-templated kernels of a library are instantiated for:
//   the default library                    every built-in model
//   -DSNN_LAB_BUILD                        Izhikevich and Hodgkin-Huxley only -- a library for kernel experiments
//                                          (profiles/experiments/README.md), a quarter of the compile time; never the library
//                                          the tests or the bench load by default
//   a library carrying generated code      the two-kernel step only (shorter compile), but for its own neuron model the
//                                          one-launch small-lattice step too
#pragma once
#include <type_traits>
#include <utility>

#include "snn_custom_model.hpp"

namespace {

template <int V> using int_c = std::integral_constant<int, V>;
template <bool V> using bool_c = std::bool_constant<V>;
template <int... Ms> struct model_list {};
template <int... Ms, int M> model_list<Ms..., M> operator+(model_list<Ms...>, int_c<M>);

#ifdef SNN_LAB_BUILD
using BuiltinModels = model_list<0, 2>;
#else
using BuiltinModels = model_list<0, 1, 2, 3, 4, 5, 6, 7>;
#endif
// k_update, k_update_wide
using UpdateModels = std::conditional_t<SNN_HAVE_CUSTOM_NEURON, decltype(BuiltinModels{} + int_c<snn::CUSTOM_MODEL>{}), BuiltinModels>;
// k_inputs_dense_close, k_run_resident, k_step_csr, k_step_csr_img
using FusedModels = std::conditional_t<SNN_HAVE_CUSTOM_MODEL, model_list<>, BuiltinModels>;
// k_step_resident, k_step_resident_q
using ResidentStepModels = std::conditional_t<SNN_HAVE_CUSTOM_MODEL && SNN_HAVE_CUSTOM_NEURON, model_list<snn::CUSTOM_MODEL>, FusedModels>;
// k_run_resident with the neuron state in registers: the models whose update that kernel carries itself (a lab build has all four)
using RunRegisterModels = std::conditional_t<SNN_HAVE_CUSTOM_MODEL, model_list<>, model_list<0, 1, 3, 4>>;
// a library carrying generated code has the generic three-slot chemical variant of k_inputs_dense only, and no input pass
// that applies STDP (shorter compile)
constexpr bool LEAN_INPUT_PASS = SNN_HAVE_CUSTOM_MODEL;

// f(int_c<M>) for the entry of the list equal to `model`, the first entry for a model the list does not have; an empty list
// calls (and instantiates) nothing
template <int First, int... Rest, class F> void for_model(model_list<First, Rest...>, int model, F &&f)
{
    if (!((model == Rest && (f(int_c<Rest>{}), true)) || ...)) f(int_c<First>{});
}
template <class F> void for_model(model_list<>, int, F &&) {}

// f(int_c<V>) for the V equal to `value`, the last V for any other value
template <int First, int... Rest, class F> void for_value(int value, F &&f)
{
    if constexpr (sizeof...(Rest) == 0) f(int_c<First>{});
    else if (value == First) f(int_c<First>{});
    else for_value<Rest...>(value, f);
}

template <class F> void for_bool(bool value, F &&f)
{
    if (value) f(bool_c<true>{});
    else f(bool_c<false>{});
}

// f(ELECTRICAL, CHEMICAL): the three pairs a stepping network can have
template <class F> void for_synapses(bool electrical, bool chemical, F &&f)
{
    if (electrical && chemical) f(bool_c<true>{}, bool_c<true>{});
    else if (electrical) f(bool_c<true>{}, bool_c<false>{});
    else f(bool_c<false>{}, bool_c<true>{});
}

} // namespace
