// biquad_i16_plan_cli — `plan_biquad_i16` (idsp_amd/csrc/biquad_i16_plan.h) from the command line, for tests/test_biquad_i16_plan.py: the
// dispatch of idsp_biquad_i16_df1 / _df1_clamp without a GPU.  Plain host C++, no HIP, no library.
//
// One case per line on stdin, one answer per line on stdout:
//   <FM|LM> <lanes> <x address> <y address> <x pitch> <y pitch> [fm_block=N]
//        -> what idsp_last_kernel() reports for that pass, a tab, `form= grid= block=`  (pitches in elements, already resolved: never 0)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../idsp_amd/csrc/biquad_i16_plan.h"

using namespace idsp::bq16;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string layout, opt;
        unsigned long long lanes = 0, x = 0, y = 0, xl = 0, yl = 0;
        if (!(in >> layout >> lanes >> x >> y >> xl >> yl) || (layout != "FM" && layout != "LM")) {
            std::printf("error: %s\n", line.c_str());
            continue;
        }
        Switches sw;
        while (in >> opt) {
            if (opt.rfind("fm_block=", 0) == 0) sw.fm_block = unsigned(std::stoul(opt.substr(9)));
        }
        const Plan p = plan_biquad_i16(layout == "LM", size_t(lanes), uintptr_t(x), uintptr_t(y), size_t(xl), size_t(yl), sw);
        std::printf("%s\tform=%d grid=%u block=%u\n", p.name, int(p.form), p.grid, p.block);
    }
    return 0;
}
