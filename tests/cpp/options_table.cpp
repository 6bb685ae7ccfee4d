// Prints what the option table of csrc/snn_options.hpp stores: per row its sources, after-effect and default, the value
// snn_set_option's rule gives for a list of ints and the value the environment's rule gives for a list of strings.
// tests/test_options_table.py compares the output with its own restatement of the rules.  Includes nothing else of the library.
#include <cstdio>
#include <vector>

#include "snn_options.hpp"

int main()
{
    using namespace snn;
    std::vector<int> ints;
    for (int v = -3; v <= 70; ++v) ints.push_back(v);
    for (int v : {INT_MIN, INT_MAX, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 26}) ints.push_back(v);
    const char *strings[] = {"", "0", "1", "2", "3", "4", "5", "6", "7", "8", "9", "12", "x", "-1", "4096"};
    static const char *const sources[] = {"option+env", "option", "env"};
    static const char *const afters[] = {"none", "x_agreed=false", "uni_dirty=true", "run_probed_grid=0"};
    const Options defaults;
    for (const OptionRow &r : OPTION_TABLE) {
        printf("row %s %s %s %s default %u\n", r.name, sources[r.source], afters[r.after],
               r.source == OPTION_ONLY ? "-" : option_env_name(r).c_str(), defaults.*r.member);
        if (r.source != ENV_ONLY)
            for (int v : ints) {
                Options o;
                o.*r.member = option_value(r, v);
                printf("opt %s %d %u\n", r.name, v, o.*r.member);
            }
        if (r.source != OPTION_ONLY)
            for (const char *e : strings) {
                Options o;
                o.*r.member = option_from_env(r, e);
                printf("env %s \"%s\" %u\n", r.name, e, o.*r.member);
            }
    }
    return 0;
}
