// combine.cpp -- the reference's examples/cpp/combine.cpp on the GPU path:
//   combine [--samples] <directory>
// aligns the .wav files of the directory (in name order) with GpuAudioCombiner::combine: the filters are learned from
// the files, every file is searched against the others, and "FINDING <file>", then "<best> <cnt> <confidence> <offset>"
// and a blank line are printed per file.  With --samples one more line per file follows all of these: the file's best
// alignment hit refined to the sample by the exact cross-correlation of the PCM (GpuAudioCombiner::refine),
// "<recording> <offset_samples> <inverted> <score>" with file[n + offset_samples] ~ recording[n], or " 0 0 0" without a hit.
#include <algorithm>
#include <cstdio>
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

int main(int argc, char **argv)
{
    std::ios_base::sync_with_stdio(false);
    std::cin.tie(nullptr);
    const bool samples = argc == 3 && std::string(argv[1]) == "--samples";
    if ((argc != 2 && !samples) || (argc == 2 && std::string(argv[1]) == "--samples")) {
        std::cerr << "usage: combine [--samples] <directory of .wav files>" << std::endl;
        return 2;
    }
    try {
        const auto files = get_filenames(argv[argc - 1]);
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
    } catch (const std::exception &e) {
        std::cerr << "combine: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
