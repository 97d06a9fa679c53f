// stream_plan_cli — `plan_stream` (idsp_amd/csrc/stream_plan.h) from the command line, for tests/test_stream_plan.py: the dispatch of
// `launch_stream` without a GPU.  Plain host C++, no HIP, no library.
//
// One case per line on stdin, one answer per line on stdout:
//   plan <traits> <lanes> <frames> <FM|LM> <x mod 64> <y mod 64> <pitch x> <pitch y> [remainder] [no_side_stream] [IDSP_SWITCH=value ...]
//        -> what idsp_last_kernel() reports for that call: `name<traits>suffixes`, a tab, the plan's launch parameters (pitches in elements,
//           0 = dense; a switch counts as set under IDSP_DIAG=1, which therefore has to be among them — exactly as in the library)
//   geom <lanes> <max_lpt>                     -> `grid x lpt x bw, rounds` of sweep_geometry, or `none`
//   duo <sections> <lanes> <FM|LM> [IDSP_SWITCH=value ...]  -> 0 / 1 of duo_wanted
//   lockin <entry> <order | n> <cascade | 0> <lanes> <frames> <FM|LM> <x mod 64> <y mod 64> [tuned] [IDSP_SWITCH=value ...]
//        -> `plan_lockin` (idsp_amd/csrc/lockin_plan.h) for a call of idsp_lockin_i32_<entry> (process, arg, norm_sqr, biquad_process, lo_process,
//           biquad_lo_process, accu_process) or idsp_lockin_f32_biquad_lo_process (f32_biquad_lo_process): what idsp_last_kernel() reports —
//           `stream_<Processor>` where launch_stream names the kernel —, a tab, `waves= groups= batch= in= skew= body= split=`
//           (tuned: stagger_tuned_device() holds)
//   hbf <dec|int> <tap_set|-1> <stages> <lanes> <frames> <FM|LM> <wide mod 16> [IDSP_SWITCH=value ...]
//        -> `plan_hbf` (idsp_amd/csrc/resample_plan.h) for a call of idsp_hbf_<dec|int>_f32: the start of what idsp_last_kernel() reports
//           (hbf_plan_name), a tab, `form= grid=`
//   cic <dec|int> <32|64> <order> <rate> <lanes> <frames> <FM|LM> <x mod 16> <y mod 16> [IDSP_SWITCH=value ...]
//        -> `plan_cic` for a call of idsp_cic_<dec|int>_i<32|64>: cic_plan_name, a tab, `form= ppt= vpc= grid=`
//   fm_disc <lanes> <frames> <FM|LM> <x mod 16> <y mod 16> [tuned] [IDSP_SWITCH=value ...]
//        -> `plan_fm_disc` (idsp_amd/csrc/readout_plan.h) for a call of idsp_fm_disc_i32: the start of what idsp_last_kernel() reports
//           (fm_disc_plan_name), a tab, `form= waves= grid= body= tail= skew= shift= mod=`
//   dds <lanes> <frames> <FM|LM> [IDSP_SWITCH=value ...]
//        -> `plan_dds` for a call of idsp_dds_i32: `stream_<Processor>`, a tab, `split= circle=`
//   passes <chain|bylane|cascade|wdf|i16> <sample bytes> <clamp 0|1> <state words> <n> <lanes> <FM|LM> [IDSP_SWITCH=value ...]
//        -> `next_pass` (idsp_amd/csrc/biquad_pass_plan.h) until the n sections of a call are done: the launches in order, `na+nb` for one of the
//           two-wave kernel and `na` for one of launch_stream, e.g. `4+4 2+2` or `4 4 1` (bytes, clamp and words are read by the families whose
//           rules take them)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../../idsp_amd/csrc/biquad_pass_plan.h"
#include "../../idsp_amd/csrc/lockin_plan.h"
#include "../../idsp_amd/csrc/readout_plan.h"
#include "../../idsp_amd/csrc/resample_plan.h"
#include "../../idsp_amd/csrc/stream_plan.h"

using namespace idsp;

// The processors, by hand.  Values the processor does not declare are the detectors' defaults (lane_stream.h: LdsEligibleOf `COST <= 120`,
// LdsRingOf 8, FmStagedOf / LmStagedOf from the sample sizes, IN_DIV and BATCH; fm_sweep.h: SweepMaxLptOf `COST <= 120 ? 4 : 2`).
static StreamTraits traits(bool has_in, int in_div, size_t in_bytes, size_t out_bytes, int cost, bool lds_eligible, int lds_ring, bool fm_staged, bool lm_staged,
                           bool lm_one_form, int sweep_max_lpt)
{
    StreamTraits t;
    t.has_in = has_in, t.in_div = in_div, t.in_bytes = in_bytes, t.out_bytes = out_bytes, t.cost = cost;
    t.lds_eligible = lds_eligible, t.lds_ring = lds_ring;
    t.fm_staged = fm_staged, t.lm_staged = lm_staged, t.lm_one_form = lm_one_form, t.sweep_max_lpt = sweep_max_lpt;
    return t;
}
static const std::map<std::string, StreamTraits> kTraits = {
    // biquad_sections.h `Chain<Df1I32<false>, N>` (COST = N * 50, LDS_RING 7 for one section else 4, LDS_ELIGIBLE = N <= LDS_MAX_N = 3,
    // SWEEP_MAX_LPT 16 / 8 / 2 for N = 1 / 2 / 3): what idsp_biquad_i32_df1 runs for n = 1, 2, 3 sections
    {"i32_df1", traits(true, 1, 4, 4, 50, true, 7, true, true, false, 16)},
    {"i32_df1_x2", traits(true, 1, 4, 4, 100, true, 4, true, true, false, 8)},
    {"i32_df1_x3", traits(true, 1, 4, 4, 150, true, 4, true, true, false, 2)},
    // biquad_sections.h `Chain<Df2tF32<false>, 1>` (COST 22, LDS_RING 7, LDS_MAX_N 2): idsp_biquad_f32_df2t, one section
    {"f32_df2t", traits(true, 1, 4, 4, 22, true, 7, true, true, false, 16)},
    // phase_procs.h `ClampWrapProc` (COST 40, nothing else declared): a cheap 4-byte processor on the detectors' defaults
    {"clamp_wrap", traits(true, 1, 4, 4, 40, true, 8, true, true, false, 4)},
    // phase_procs.h `PllProc<0>` (COST 160, nothing else declared): a heavy 4-byte processor that is not LDS-eligible
    {"pll", traits(true, 1, 4, 4, 160, false, 8, true, true, false, 2)},
    // rpll_procs.h `RpllProc` (8-byte samples in and out, COST 150, nothing else declared)
    {"rpll", traits(true, 1, 8, 8, 150, false, 8, true, true, false, 2)},
    // phase_procs.h `UnwrapProc<1>` (int32 in, int64 out, COST 16, LDS_ELIGIBLE = false): an 8-byte output
    {"unwrap_i64", traits(true, 1, 4, 8, 16, false, 8, false, false, false, 4)},
    // lockin_stream_procs.h `LockinSplitProc<2, 2>` (IN_DIV 2, COST 70 + 40 * 4, BATCH 4): two threads share an input lane
    {"lockin_split", traits(true, 2, 4, 4, 230, false, 8, false, false, false, 2)},
};

// name / also: what the launcher records; detail: the launch parameters of the plan that named the kernel
static void print_plan(const StreamTraits &t, StreamCall c, const StreamSwitches &sw, std::string &name, std::string &also, std::string &detail)
{
    StreamPlan p = plan_stream(t, c, sw);
    if (p.form == StreamForm::FmOddBeside) {
        print_plan(t, lane_block(c, p, 0, p.body, false), sw, name, also, detail);  // the body records the name ...
        also += stream_plan_also(p);                                                // ... and the few kernel is appended to it
        return;
    }
    if (p.form == StreamForm::FmRoundsBeside) p.head_swept = plan_stream(t, lane_block(c, p, 0, p.head, false), sw).form == StreamForm::FmSweep;
    name = stream_plan_name(p);
    also = stream_plan_also(p) ? stream_plan_also(p) : "";
    char text[256];
    snprintf(text, sizeof text, "grid=%u lanes_per_wave=%d deep_ring=%d xcdc=%d staged_flags=%d block=%u deep_window=%d head=%zu tail=%zu sweep=%ux%dx%u,%u,fps%u",
             p.grid, p.lanes_per_wave, int(p.deep_ring), int(p.xcdc), p.staged_flags, p.block, int(p.deep_window), p.head, p.tail, p.geom.grid,
             p.geom.lpt, p.geom.bw, p.geom.rounds, p.geom.fps);
    detail = text;
}

// The lock-in entries, by hand: arms and LO of each, the stream processor it runs (lockin_phase.hip, lockin_generic.hip, lockin_accu.hip) and the
// name of its arm functor on the multi-wave kernel (`Bank::name()`: lockin_waves_biquad.hip, lockin_waves_lo.hip; none for `LpBank`)
static bool lockin_line(std::istringstream &in, const LockinSwitches &sw, bool tuned, const std::string &entry, std::string &out)
{
    static const std::map<std::string, int> kEntries = {{"process", 0}, {"arg", 1}, {"norm_sqr", 2}, {"biquad_process", 3}, {"lo_process", 4},
                                                        {"biquad_lo_process", 5}, {"f32_biquad_lo_process", 6}, {"accu_process", 7}};
    int a = 0, b = 0;
    size_t xo = 0, yo = 0;
    std::string layout;
    LockinCall c;
    in >> a >> b >> c.lanes >> c.frames >> layout >> xo >> yo;
    if (!in || !kEntries.count(entry) || (layout != "FM" && layout != "LM")) return false;
    const int e = kEntries.at(entry);
    c.arms = e == 3 || e == 5 || e == 6 ? LockinArms::Biquad : LockinArms::Lowpass;
    c.lo = e <= 3 ? LockinLo::Phase : e == 7 ? LockinLo::Accu : LockinLo::Buffer;
    c.readout = e == 1 ? MODE_ARG : e == 2 ? MODE_NORM_SQR : MODE_IQ;
    if (c.arms == LockinArms::Lowpass) c.order = a, c.cascade = b;
    c.layout = layout == "LM" ? IDSP_LANE_MAJOR : IDSP_FRAME_MAJOR;
    c.x = (uintptr_t(1) << 32) + xo, c.y = (uintptr_t(1) << 33) + yo;
    c.tuned_device = tuned;
    const LockinPlan p = plan_lockin(c, sw);
    char proc[96], bank[64] = "", text[512];
    const char *const procs[8] = {p.split ? "LockinSplitProc<%d, %d>" : "LockinProc<%d, %d>", "LockinPolarProc<%d, %d, 0>", "LockinPolarProc<%d, %d, 1>", "LockinBiquadProc<%d>",
                                  "LockinLoProc<%d, %d>", "LockinBiquadLoProc<idsp::bq::Df1I32<false>, %d>", "LockinBiquadLoProc<idsp::bq::Df1F32<false>, %d>",
                                  p.split ? "LockinAccuSplitProc<%d, %d>" : "LockinAccuProc<%d, %d>"};
    const char *const banks[8] = {"", "", "", "[Biquad; %d]", "[Lowpass<N>; K], LO", "[Biquad; %d], LO", "[Biquad<f32>; %d], LO", ""};
    snprintf(proc, sizeof proc, procs[e], a, b);
    snprintf(bank, sizeof bank, banks[e], a);
    // the entries with an LO buffer leave the name of the tail's stream launch; the biquad phase entry records the combined one with "[Biquad; n]"
    const bool streams = p.form == LockinForm::Stream || (p.form == LockinForm::WavesTail && c.lo == LockinLo::Buffer);
    const char *detail = streams ? proc : p.form == LockinForm::Waves ? bank : p.form == LockinForm::WavesTail && e == 3 ? "[Biquad; n]" : "";
    static const char *const kIn[5] = {"-", "FM_REG", "FM_DMA", "LM_REG", "LM_DMA"};
    snprintf(text, sizeof text, "%s%s%s%s\twaves=%d groups=%d batch=%d in=%s skew=%u body=%zu split=%d", streams ? "stream_" : lockin_plan_name(p), *detail ? "<" : "", detail,
             *detail ? ">" : "", p.waves, p.groups, p.batch, kIn[p.in + 1], p.skew, p.body, int(p.split));
    out = text;
    return true;
}

// the two resampling verbs: the shape words of the line, then the switches
template <class Env>
static bool resample_line(const std::string &cmd, std::istringstream &in, std::map<std::string, std::string> &env, Env getenv_, std::string &out)
{
    std::string kind, layout, word;
    int bits = 32;
    HbfCall h;
    CicCall c;
    size_t xo = 0, yo = 0;
    in >> kind;
    if (cmd == "hbf")
        in >> h.tap_set >> h.stages >> h.lanes >> h.frames >> layout >> xo;
    else
        in >> bits >> c.order >> c.rate >> c.lanes >> c.frames >> layout >> xo >> yo;
    if (!in || (kind != "dec" && kind != "int") || (layout != "FM" && layout != "LM") || (bits != 32 && bits != 64)) return false;
    while (in >> word) {
        if (word.find('=') == std::string::npos) return false;
        env[word.substr(0, word.find('='))] = word.substr(word.find('=') + 1);
    }
    char text[256];
    if (cmd == "hbf") {
        h.dec = kind == "dec", h.layout = layout == "LM" ? IDSP_LANE_MAJOR : IDSP_FRAME_MAJOR, h.wide = (uintptr_t(1) << 32) + xo;
        static const char *const kForms[6] = {"Generic", "BlkLm", "RingFm", "BlockFm", "WaveFm", "WaveLm"};
        const HbfPlan p = plan_hbf(h, read_hbf_switches(getenv_));
        snprintf(text, sizeof text, "%s\tform=%s grid=%u", hbf_plan_name(p), kForms[int(p.form)], p.grid);
    } else {
        c.dec = kind == "dec", c.elem_bytes = bits / 8, c.layout = layout == "LM" ? IDSP_LANE_MAJOR : IDSP_FRAME_MAJOR;
        c.x = (uintptr_t(1) << 32) + xo, c.y = (uintptr_t(1) << 33) + yo;
        static const char *const kForms[4] = {"RingLm", "RingFm", "LaneTiles", "Lane"};
        const CicPlan p = plan_cic(c, read_cic_switches(getenv_));
        snprintf(text, sizeof text, "%s\tform=%s ppt=%d vpc=%d grid=%u", cic_plan_name(p), kForms[int(p.form)], p.ppt, p.vpc, p.grid);
    }
    out = text;
    return true;
}

// the two read-out verbs: the shape words of the line, `tuned`, then the switches
template <class Env>
static bool readout_line(const std::string &cmd, std::istringstream &in, std::map<std::string, std::string> &env, Env getenv_, std::string &out)
{
    std::string layout, word;
    size_t lanes = 0, frames = 0, xo = 0, yo = 0;
    bool tuned = false;
    in >> lanes >> frames >> layout;
    if (cmd == "fm_disc") in >> xo >> yo;
    if (!in || (layout != "FM" && layout != "LM")) return false;
    while (in >> word) {
        if (word == "tuned" && cmd == "fm_disc")
            tuned = true;
        else if (word.find('=') == std::string::npos)
            return false;
        else
            env[word.substr(0, word.find('='))] = word.substr(word.find('=') + 1);
    }
    char text[256];
    if (cmd == "fm_disc") {
        FmDiscCall c;
        c.lanes = lanes, c.frames = frames, c.layout = layout == "LM" ? IDSP_LANE_MAJOR : IDSP_FRAME_MAJOR;
        c.x = (uintptr_t(1) << 32) + xo, c.y = (uintptr_t(1) << 33) + yo, c.tuned_device = tuned;
        static const char *const kForms[4] = {"Stream", "WavesFm", "WavesLm", "WavesLmTail"};
        const FmDiscPlan p = plan_fm_disc(c, read_fm_disc_switches(getenv_));
        snprintf(text, sizeof text, "%s\tform=%s waves=%d grid=%u body=%zu tail=%zu skew=%u shift=%u mod=%u", fm_disc_plan_name(p), kForms[int(p.form)], p.front_waves,
                 p.grid, p.body, p.tail, p.skew, p.skew_shift, p.skew_mod);
    } else {
        DdsCall c;
        c.lanes = lanes, c.frames = frames, c.layout = layout == "LM" ? IDSP_LANE_MAJOR : IDSP_FRAME_MAJOR;
        const DdsPlan p = plan_dds(c, read_dds_switches(getenv_));
        // the stream processor the entry instantiates for the plan (dds.hip), by hand
        const char *proc = p.circle ? "DdsSplitProcT<true>" : p.split ? "DdsSplitProcT<false>" : "DdsProcT<false>";
        snprintf(text, sizeof text, "stream_<%s>\tsplit=%d circle=%d", proc, int(p.split), int(p.circle));
    }
    out = text;
    return true;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, word;
        if (!(in >> cmd)) continue;
        std::map<std::string, std::string> env;
        auto getenv_ = [&](const char *name) -> const char * {
            const auto diag = env.find("IDSP_DIAG");
            if (diag == env.end() || atoi(diag->second.c_str()) == 0) return nullptr;  // common.h `diag_env`
            const auto it = env.find(name);
            return it == env.end() ? nullptr : it->second.c_str();
        };
        if (cmd == "geom") {
            size_t lanes = 0;
            int max_lpt = 0;
            in >> lanes >> max_lpt;
            SweepGeom g;
            if (sweep_geometry(lanes, max_lpt, g))
                printf("%u x %d x %u, %u\n", g.grid, g.lpt, g.bw, g.rounds);
            else
                printf("none\n");
        } else if (cmd == "duo") {
            size_t m = 0, lanes = 0;
            std::string layout;
            in >> m >> lanes >> layout;
            while (in >> word) env[word.substr(0, word.find('='))] = word.find('=') == std::string::npos ? "" : word.substr(word.find('=') + 1);
            printf("%d\n", int(duo_wanted(m, lanes, layout == "LM" ? IDSP_LANE_MAJOR : IDSP_FRAME_MAJOR, read_stream_switches(getenv_))));
        } else if (cmd == "passes") {
            std::string family, layout;
            size_t bytes = 0, n = 0, lanes = 0;
            int clamp = 0, words = 0;
            in >> family >> bytes >> clamp >> words >> n >> lanes >> layout;
            static const std::map<std::string, int> kFamilies = {{"chain", 0}, {"bylane", 1}, {"cascade", 2}, {"wdf", 3}, {"i16", 4}};
            if (!in || !kFamilies.count(family) || (layout != "FM" && layout != "LM")) {
                printf("error: %s\n", line.c_str());
                continue;
            }
            while (in >> word) env[word.substr(0, word.find('='))] = word.find('=') == std::string::npos ? "" : word.substr(word.find('=') + 1);
            const PassRules rules[5] = {chain_rules(bytes, clamp != 0, words), bylane_rules(bytes), cascade_rules(bytes), wdf_rules(), i16_rules()};
            const PassRules &r = rules[kFamilies.at(family)];
            const StreamSwitches sw = read_stream_switches(getenv_);
            std::string out;
            for (size_t done = 0; done < n;) {
                const Pass p = next_pass(r, n - done, lanes, layout == "LM" ? IDSP_LANE_MAJOR : IDSP_FRAME_MAJOR, sw);
                if (p.na + p.nb <= 0) break;  // (no rule does that: the line would not end)
                out += (done ? " " : "") + std::to_string(p.na) + (p.nb ? "+" + std::to_string(p.nb) : "");
                done += size_t(p.na + p.nb);
            }
            printf("%s\n", out.c_str());
        } else if (cmd == "lockin") {
            std::string entry, rest, out;
            in >> entry;
            std::getline(in, rest);
            bool tuned = false;
            std::string shape;
            std::istringstream words(rest);
            while (words >> word) {
                if (word == "tuned")
                    tuned = true;
                else if (word.find('=') != std::string::npos)
                    env[word.substr(0, word.find('='))] = word.substr(word.find('=') + 1);
                else
                    shape += word + " ";
            }
            std::istringstream shape_in(shape);
            if (lockin_line(shape_in, read_lockin_switches(getenv_), tuned, entry, out))
                printf("%s\n", out.c_str());
            else
                printf("error: %s\n", line.c_str());
        } else if (cmd == "hbf" || cmd == "cic") {
            std::string out;
            if (resample_line(cmd, in, env, getenv_, out))
                printf("%s\n", out.c_str());
            else
                printf("error: %s\n", line.c_str());
        } else if (cmd == "fm_disc" || cmd == "dds") {
            std::string out;
            if (readout_line(cmd, in, env, getenv_, out))
                printf("%s\n", out.c_str());
            else
                printf("error: %s\n", line.c_str());
        } else if (cmd == "plan") {
            std::string tn, layout;
            StreamCall c;
            size_t xo = 0, yo = 0;
            in >> tn >> c.lanes >> c.frames >> layout >> xo >> yo >> c.pitch_x >> c.pitch_y;
            if (!in || !kTraits.count(tn) || (layout != "FM" && layout != "LM")) {
                printf("error: %s\n", line.c_str());
                continue;
            }
            c.layout = layout == "LM" ? IDSP_LANE_MAJOR : IDSP_FRAME_MAJOR;
            c.x = (uintptr_t(1) << 32) + xo, c.y = (uintptr_t(1) << 33) + yo;
            while (in >> word) {
                if (word == "remainder")
                    c.remainder_of_split = true;
                else if (word == "no_side_stream")
                    c.no_side_stream = true;
                else
                    env[word.substr(0, word.find('='))] = word.find('=') == std::string::npos ? "" : word.substr(word.find('=') + 1);
            }
            std::string name, also, detail;
            print_plan(kTraits.at(tn), c, read_stream_switches(getenv_), name, also, detail);
            printf("%s<%s>%s\t%s\n", name.c_str(), tn.c_str(), also.c_str(), detail.c_str());
        } else {
            printf("error: %s\n", line.c_str());
        }
    }
    return 0;
}
