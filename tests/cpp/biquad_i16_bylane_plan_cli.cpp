// biquad_i16_bylane_plan_cli — `plan_biquad_i16_bylane` beside `plan_biquad_i16` (idsp_amd/csrc/biquad_i16_plan.h) from the command line,
// for tests/test_biquad_i16_bylane_host.py: the dispatch of idsp_biquad_i16_df1_bylane / _df1_clamp_bylane without a GPU.  Plain host
// C++, no HIP, no library.
//
// One case per line on stdin, one answer per line on stdout:
//   <FM|LM> <lanes> <x address> <y address> <x pitch> <y pitch> [fm_block=N]
//        -> the by-lane kernel name, a tab, the shared entry's kernel name, a tab, `form= grid= block= same=` (same: the two plans agree
//           in form, grid and block)
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
        const Plan s = plan_biquad_i16(layout == "LM", size_t(lanes), uintptr_t(x), uintptr_t(y), size_t(xl), size_t(yl), sw);
        const Plan p = plan_biquad_i16_bylane(layout == "LM", size_t(lanes), uintptr_t(x), uintptr_t(y), size_t(xl), size_t(yl), sw);
        std::printf("%s\t%s\tform=%d grid=%u block=%u same=%d\n", p.name, s.name, int(p.form), p.grid, p.block,
                    int(p.form == s.form && p.grid == s.grid && p.block == s.block));
    }
    return 0;
}
