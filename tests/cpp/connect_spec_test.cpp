// LatticeNetworkGPU::connect(snn_connect_spec) and ::connect_sparse(std::vector<snn_connect_spec>) of the C++ host mirror
// (spiking-neural-networks_amd/host/snn_lattice.hpp) on the ragged network of the Python tests -- neurons 3x5 and 5x7, 2x3 rate
// cells -- with the four records of tests/connect_spec_cases.py: argv[1] is a file that the Python restatement wrote, per record
//   pre post rule extent self_edges probability edge_seed weight_rule w_lo w_hi weight_seed wrap table_rows table_cols
// followed by the table_rows * table_cols entries; every float is written as the hexadecimal pattern of its bits.  The program applies them to a dense handle one by
// one and to a sparse handle as one batch, and prints FNV-1a digests of what it reads back -- dense: weight bits, then connection
// flags of all rows; sparse: row_ptr, pre_index, weight bits -- for tests/test_gpu_connect_spec_cpp.py to compare.
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../spiking-neural-networks_amd/host/snn_lattice.hpp"

using namespace snn_host;

struct Digest {
    uint64_t h = 0xcbf29ce484222325ull;
    void eat(uint64_t word, int bytes) { for (int b = 0; b < bytes; ++b) { h ^= (word >> (8 * b)) & 0xffu; h *= 0x100000001b3ull; } }
};

int main(int argc, char **argv)
{
    if (argc < 2) return 64;
    try {
        std::ifstream in(argv[1]);
        std::vector<snn_connect_spec> specs;
        std::vector<std::vector<float>> tables;
        snn_connect_spec s{};
        auto real = [&in](float &x) {
            uint32_t bits = 0;
            in >> std::hex >> bits >> std::dec;
            std::memcpy(&x, &bits, 4);
        };
        while (in >> s.record.pre_id >> s.record.post_id >> s.record.rule >> s.record.extent >> s.record.self_edges) {
            real(s.record.probability);
            in >> s.record.edge_seed >> s.record.weight_rule;
            real(s.record.w_lo);
            real(s.record.w_hi);
            in >> s.record.weight_seed >> s.wrap >> s.table_rows >> s.table_cols;
            std::vector<float> table((size_t)s.table_rows * s.table_cols);
            for (float &x : table) real(x);
            tables.push_back(std::move(table));
            specs.push_back(s);
        }
        for (size_t k = 0; k < specs.size(); ++k) specs[k].table = tables[k].empty() ? nullptr : tables[k].data();
        if (specs.size() != 4) { std::fprintf(stderr, "%zu records read\n", specs.size()); return 2; }

        IzhikevichNeuron base;
        LatticeNetwork<IzhikevichNeuron, RateSpikeTrain> net;
        Lattice<IzhikevichNeuron> a, b;
        a.set_id(0);
        a.populate(base, 3, 5);
        b.set_id(1);
        b.populate(base, 5, 7);
        SpikeTrainLattice<RateSpikeTrain> cells;
        cells.set_id(2);
        cells.populate(RateSpikeTrain(), 2, 3);
        net.add_lattice(a);
        net.add_lattice(b);
        net.add_spike_train_lattice(cells);

        auto dense = LatticeNetworkGPU<IzhikevichNeuron, RateSpikeTrain>::from_network(net);
        for (const auto &spec : specs) dense.connect(spec);
        std::vector<float> w(56 * 50);
        std::vector<uint32_t> c(56 * 50);
        check(snn_get_graph_rows(dense.handle(), 0, 56, w.data(), c.data()));
        Digest d;
        for (float x : w) { uint32_t bits; std::memcpy(&bits, &x, 4); d.eat(bits, 4); }
        for (uint32_t x : c) d.eat(x, 4);
        size_t edges = 0;
        for (uint32_t x : c) edges += x != 0;

        auto sparse = LatticeNetworkGPU<IzhikevichNeuron, RateSpikeTrain>::from_network_sparse(net);
        sparse.connect_sparse(specs);
        const auto structure = sparse.csr_structure();
        const auto weights = sparse.csr_weights();
        Digest e;
        for (uint64_t x : structure.first) e.eat(x, 8);
        for (uint32_t x : structure.second) e.eat(x, 4);
        for (float x : weights) { uint32_t bits; std::memcpy(&bits, &x, 4); e.eat(bits, 4); }

        // a refused spec throws and names its argument
        bool thrown = false;
        snn_connect_spec bad = specs[0];
        bad.wrap = 4;
        try { dense.connect(bad); } catch (const GPUError &err) { thrown = err.code == SNN_ERR_BAD_ARG && std::strstr(err.what(), "wrap"); }
        if (!thrown) { std::fprintf(stderr, "wrap = 4 did not throw GPUError(SNN_ERR_BAD_ARG) naming wrap\n"); return 3; }
        std::printf("dense %016llx edges %zu sparse %016llx nnz %zu\n", (unsigned long long)d.h, edges, (unsigned long long)e.h, weights.size());
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
