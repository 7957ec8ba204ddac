// combine.cpp -- the reference's examples/cpp/combine.cpp on the GPU path:
//   combine [--samples [--render <out.wav>] [--tracks <dir>] [--min-peak N] [--min-score X] [--anchor-hop N] [--radius N]] <directory>
// aligns the .wav files of the directory (in name order) with GpuAudioCombiner::combine: the filters are learned from
// the files, every file is searched against the others, and "FINDING <file>", then "<best> <cnt> <confidence> <offset>"
// and a blank line are printed per file.  With --samples one more line per file follows all of these: the file's best
// alignment hit refined to the sample by the exact cross-correlation of the PCM (GpuAudioCombiner::refine),
// "<recording> <offset_samples> <inverted> <score>" with file[n + offset_samples] ~ recording[n], or " 0 0 0" without a hit.
// With --render or --tracks (after --samples) the recordings are then placed with their clock drift
// (GpuAudioCombiner::layout_drift; --min-peak 20, --min-score 0.5, --anchor-hop 2097152 and --radius 1024 unless given), one
// line "<members> : <start> <rate> ..." is printed per component, and the component with the most members (the first of
// them) is rendered: its mix to <out.wav>, every member alone to <dir>/track<k>.wav (PCM16 mono at 44.1 kHz).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <iostream>
#include <string>
#include <vector>

#include <hpfw/gpu/audio_combiner.h>

namespace fs = std::filesystem;

static std::vector<std::string> get_filenames(const std::string &dir)
{
    std::vector<std::string> files;
    for (const auto &f : fs::directory_iterator(dir)) {
        if (f.path().extension() != ".wav") continue;
        files.emplace_back(f.path().string());
    }
    std::sort(files.begin(), files.end()); // the reference's directory order is unspecified
    return files;
}

static int usage()
{
    std::cerr << "usage: combine [--samples [--render <out.wav>] [--tracks <dir>] [--min-peak N] [--min-score X] [--anchor-hop N] [--radius N]] "
                 "<directory of .wav files>"
              << std::endl;
    return 2;
}

int main(int argc, char **argv)
{
    std::ios_base::sync_with_stdio(false);
    std::cin.tie(nullptr);
    bool samples = false;
    std::string render, tracks, dir;
    long min_peak = 20, anchor_hop = 1l << 21, radius = 1024;
    double min_score = 0.5;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool more = i + 2 < argc; // a value and the directory follow
        if (a == "--samples") samples = true;
        else if (a == "--render" && more) render = argv[++i];
        else if (a == "--tracks" && more) tracks = argv[++i];
        else if (a == "--min-peak" && more) min_peak = std::atol(argv[++i]);
        else if (a == "--min-score" && more) min_score = std::atof(argv[++i]);
        else if (a == "--anchor-hop" && more) anchor_hop = std::atol(argv[++i]);
        else if (a == "--radius" && more) radius = std::atol(argv[++i]);
        else if (i == argc - 1 && a.rfind("--", 0) != 0) dir = a;
        else return usage();
    }
    const bool drift = !render.empty() || !tracks.empty();
    if (dir.empty() || (drift && !samples)) return usage();
    try {
        const auto files = get_filenames(dir);
        hpfw::GpuAudioCombiner combiner;
        combiner.set_keep_audio(samples);
        combiner.combine(files);
        for (size_t i = 0; samples && i < files.size(); ++i) {
            const auto hits = combiner.align(combiner.hashprints_of(files[i]), 1, (int)i);
            const auto fine = combiner.refine(files[i], hits);
            char score[40] = "0";
            if (!fine.empty()) std::snprintf(score, sizeof score, "%.17g", fine[0].score);
            std::cout << (fine.empty() ? std::string() : fine[0].filename) << " " << (fine.empty() ? 0 : fine[0].offset_samples) << " "
                      << (fine.empty() ? 0 : (int)fine[0].inverted) << " " << score << std::endl;
        }
        if (drift) {
            const auto comps = combiner.layout_drift((uint32_t)min_peak, min_score, 8, (int64_t)1 << 16, anchor_hop, (int)radius);
            size_t best = 0;
            for (size_t c = 0; c < comps.size(); ++c) {
                if (comps[c].members.size() > comps[best].members.size()) best = c;
                for (size_t k = 0; k < comps[c].members.size(); ++k) {
                    char line[120];
                    std::snprintf(line, sizeof line, "%s%d : %.17g %.17g", k ? " " : "", comps[c].members[k], comps[c].starts[k], comps[c].rates[k]);
                    std::cout << line;
                }
                std::cout << std::endl;
            }
            if (comps.empty()) throw std::runtime_error("nothing to render");
            const auto check = [](int rc) {
                if (rc != 0) throw std::runtime_error(hpfw_gpu_last_error());
            };
            if (!render.empty()) {
                const auto mix = combiner.render(comps[best]);
                check(hpfw_gpu_wav_write_pcm16(render.c_str(), mix.data(), (int64_t)mix.size(), 1));
            }
            if (!tracks.empty()) {
                const auto all = combiner.render(comps[best], {}, true);
                const size_t n = comps[best].members.size(), len = n ? all.size() / n : 0;
                fs::create_directories(tracks);
                for (size_t k = 0; k < n; ++k)
                    check(hpfw_gpu_wav_write_pcm16((fs::path(tracks) / ("track" + std::to_string(k) + ".wav")).string().c_str(), all.data() + k * len,
                                                   (int64_t)len, 1));
            }
        }
    } catch (const std::exception &e) {
        std::cerr << "combine: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
