// cache_files.cpp -- see cache_files.h
#include "cache_files.h"

#include <filesystem>
#include <fstream>

#include "../../include/hpfw_gpu.h" // the dimensions

namespace hpfw {

bool write_matrix(const std::string &path, int32_t rows, int32_t cols, const float *colmajor)
{
    std::ofstream os(path, std::ios::binary);
    if (!os) return false;
    os.write(reinterpret_cast<const char *>(&rows), 4);
    os.write(reinterpret_cast<const char *>(&cols), 4);
    os.write(reinterpret_cast<const char *>(colmajor), (std::streamsize)rows * cols * 4);
    return (bool)os;
}

bool read_matrix(const std::string &path, int32_t rows, int32_t &cols, std::vector<float> &colmajor)
{
    std::ifstream is(path, std::ios::binary);
    if (!is) return false;
    const bool any_cols = cols < 0;
    int32_t r = 0, c = 0;
    is.read(reinterpret_cast<char *>(&r), 4);
    is.read(reinterpret_cast<char *>(&c), 4);
    if (any_cols) cols = c;
    if (!is || r != rows || (any_cols ? c < 0 || c > (1 << 24) : c != cols)) return false;
    std::error_code ec;
    if (any_cols && (std::filesystem::file_size(path, ec) != (uintmax_t)8 + (uintmax_t)r * c * 4 || ec)) return false;
    colmajor.resize((size_t)r * c);
    is.read(reinterpret_cast<char *>(colmajor.data()), (std::streamsize)colmajor.size() * 4);
    return (bool)is;
}

bool load_filters_cereal(const std::string &path, std::vector<float> &f)
{
    int32_t cols = HPFW_FRAME_SIZE;
    return read_matrix(path, HPFW_FILTERS, cols, f);
}

bool save_filters_cereal(const std::string &path, const std::vector<float> &f)
{
    return write_matrix(path, HPFW_FILTERS, HPFW_FRAME_SIZE, f.data());
}

bool load_cov_cereal(const std::string &path, std::vector<float> &cov)
{
    int32_t cols = HPFW_FRAME_SIZE;
    return read_matrix(path, HPFW_FRAME_SIZE, cols, cov);
}

bool save_cov_cereal(const std::string &path, const std::vector<float> &cov)
{
    return write_matrix(path, HPFW_FRAME_SIZE, HPFW_FRAME_SIZE, cov.data());
}

bool save_spectro_cereal(const std::string &path, const float *binmajor, int32_t cols)
{
    std::vector<float> cm((size_t)HPFW_BINS * cols);
    for (int32_t b = 0; b < HPFW_BINS; ++b)
        for (int32_t c = 0; c < cols; ++c) cm[(size_t)c * HPFW_BINS + b] = binmajor[(size_t)b * cols + c];
    return write_matrix(path, HPFW_BINS, cols, cm.data());
}

bool load_spectro_cereal(const std::string &path, std::vector<float> &colmajor, int32_t &cols)
{
    cols = -1;
    return read_matrix(path, HPFW_BINS, cols, colmajor);
}

} // namespace hpfw
