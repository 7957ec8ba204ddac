// combine.cpp -- the reference's examples/cpp/combine.cpp on the GPU path:
//   combine <directory>
// aligns the .wav files of the directory (in name order) with GpuAudioCombiner::combine: the filters are learned from
// the files, every file is searched against the others, and "FINDING <file>", then "<best> <cnt> <confidence> <offset>"
// and a blank line are printed per file.
#include <algorithm>
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
    if (argc != 2) {
        std::cerr << "usage: combine <directory of .wav files>" << std::endl;
        return 2;
    }
    try {
        const auto files = get_filenames(argv[1]);
        hpfw::GpuAudioCombiner combiner;
        combiner.combine(files);
    } catch (const std::exception &e) {
        std::cerr << "combine: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
