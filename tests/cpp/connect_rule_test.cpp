// LatticeNetworkGPU::connect_by_rule of the C++ host mirror (spiking-neural-networks_amd/host/snn_lattice.hpp): a 4x4 lattice is
// connected by rule on the device; the program prints an FNV-1a digest of the rows (weight bits, then connection flags) that
// tests/test_gpu_connect_rule.py compares with the per-pair expectation, and checks that a refused call throws GPUError.
#include <cstdio>
#include <cstring>

#include "../../spiking-neural-networks_amd/host/snn_lattice.hpp"

using namespace snn_host;

int main()
{
    try {
        IzhikevichNeuron base;
        Lattice<IzhikevichNeuron> lattice;
        lattice.populate(base, 4, 4);
        LatticeNetwork<IzhikevichNeuron, RateSpikeTrain> net;
        net.add_lattice(lattice);
        auto gpu = LatticeNetworkGPU<IzhikevichNeuron, RateSpikeTrain>::from_network(net);
        // Euclidean radius^2 2 without self edges, thinned to 3/4, uniform weights
        gpu.connect_by_rule(0, 0, SNN_RULE_EUCLIDEAN, 2, false, 0.75f, 11, SNN_WEIGHT_UNIFORM, 0.25f, 1.75f, 5);
        std::vector<float> w(16 * 16);
        std::vector<uint32_t> c(16 * 16);
        check(snn_get_graph_rows(gpu.handle(), 0, 16, w.data(), c.data()));
        uint64_t h = 0xcbf29ce484222325ull;
        auto eat = [&h](uint32_t word) {
            for (int b = 0; b < 4; ++b) { h ^= (word >> (8 * b)) & 0xffu; h *= 0x100000001b3ull; }
        };
        for (float x : w) { uint32_t bits; std::memcpy(&bits, &x, 4); eat(bits); }
        for (uint32_t x : c) eat(x);
        size_t edges = 0;
        for (uint32_t x : c) edges += x != 0;
        // the host copy follows on sync()
        gpu.sync();
        size_t host_edges = 0;
        for (const auto &row : gpu.network.lattices.at(0).graph.matrix) for (const auto &e : row) host_edges += e.has_value();
        if (host_edges != edges) { std::fprintf(stderr, "host copy holds %zu edges, the device %zu\n", host_edges, edges); return 2; }
        bool thrown = false;
        try { gpu.connect_by_rule(0, 7, SNN_RULE_ALL); } catch (const GPUError &e) { thrown = e.code == SNN_ERR_BAD_ARG; }
        if (!thrown) { std::fprintf(stderr, "an unknown lattice id did not throw GPUError(SNN_ERR_BAD_ARG)\n"); return 3; }
        std::printf("digest %016llx edges %zu\n", (unsigned long long)h, edges);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
