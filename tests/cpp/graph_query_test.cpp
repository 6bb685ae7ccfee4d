// The Graph trait of the C++ host mirror on the device matrix (spiking-neural-networks_amd/host/snn_lattice.hpp:
// LatticeNetworkGPU::lookup_weight / edit_weight / incoming_connections / outgoing_connections): a 4x4 lattice is connected by
// rule on the device, three edges are edited, and the program prints an FNV-1a digest of the rows (weight bits, then connection
// flags) that tests/test_gpu_graph_query_cpp.py compares with the per-pair expectation -- after it has held every lookup and
// every column / row list to those rows itself.
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
        gpu.connect_by_rule(0, 0, SNN_RULE_EUCLIDEAN, 2, false, 0.75f, 11, SNN_WEIGHT_UNIFORM, 0.25f, 1.75f, 5);
        gpu.edit_weight(0, 0, 2.5f);             // a self edge the rule does not give
        gpu.edit_weight(15, 3, -1.0f);           // far apart
        gpu.edit_weight(5, 5, 9.0f);
        gpu.edit_weight(5, 5, std::nullopt);     // and gone again
        std::vector<float> w(16 * 16);
        std::vector<uint32_t> c(16 * 16);
        check(snn_get_graph_rows(gpu.handle(), 0, 16, w.data(), c.data()));
        for (uint32_t p = 0; p < 16; ++p) {
            const auto out = gpu.outgoing_connections(p);
            const auto in = gpu.incoming_connections(p);
            size_t k_out = 0, k_in = 0;
            for (uint32_t q = 0; q < 16; ++q) {
                const auto e = gpu.lookup_weight(p, q);
                if (e.has_value() != (c[p * 16 + q] != 0) || (e && std::memcmp(&*e, &w[p * 16 + q], 4))) {
                    std::fprintf(stderr, "lookup_weight(%u, %u) differs from the rows\n", p, q);
                    return 2;
                }
                if (c[p * 16 + q] && (k_out >= out.first.size() || out.first[k_out] != q || std::memcmp(&out.second[k_out], &w[p * 16 + q], 4))) {
                    std::fprintf(stderr, "outgoing_connections(%u) differs from the rows at %u\n", p, q);
                    return 3;
                }
                k_out += c[p * 16 + q] != 0;
                if (c[q * 16 + p] && (k_in >= in.first.size() || in.first[k_in] != q || std::memcmp(&in.second[k_in], &w[q * 16 + p], 4))) {
                    std::fprintf(stderr, "incoming_connections(%u) differs from the rows at %u\n", p, q);
                    return 4;
                }
                k_in += c[q * 16 + p] != 0;
            }
            if (k_out != out.first.size() || k_in != in.first.size()) { std::fprintf(stderr, "a list of %u is too long\n", p); return 5; }
        }
        bool thrown = false;
        try { gpu.lookup_weight(16, 0); } catch (const GPUError &e) { thrown = e.code == SNN_ERR_BAD_ARG; }
        if (!thrown) { std::fprintf(stderr, "an index outside the matrix did not throw GPUError(SNN_ERR_BAD_ARG)\n"); return 6; }
        uint64_t h = 0xcbf29ce484222325ull;
        auto eat = [&h](uint32_t word) {
            for (int b = 0; b < 4; ++b) { h ^= (word >> (8 * b)) & 0xffu; h *= 0x100000001b3ull; }
        };
        for (float x : w) { uint32_t bits; std::memcpy(&bits, &x, 4); eat(bits); }
        for (uint32_t x : c) eat(x);
        size_t edges = 0;
        for (uint32_t x : c) edges += x != 0;
        std::printf("digest %016llx edges %zu\n", (unsigned long long)h, edges);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
