// cache_files.h -- the files of the reference's cache directory (include/hpfw/cache.h:30-36), each cereal's binary image
// of an Eigen matrix (include/hpfw/utils.h:84-90): int32 rows, int32 cols, column-major float payload.  Host-only.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace hpfw {

bool write_matrix(const std::string &path, int32_t rows, int32_t cols, const float *colmajor);
// a matrix of `rows` rows and, cols >= 0 on entry: that many columns; cols < 0: any number up to 2^24 (returned in cols)
// in a file exactly as long as its header says
bool read_matrix(const std::string &path, int32_t rows, int32_t &cols, std::vector<float> &colmajor);

// <cache>/filters.cereal: 64 x 2420
bool load_filters_cereal(const std::string &path, std::vector<float> &f);
bool save_filters_cereal(const std::string &path, const std::vector<float> &f);
// <cache>/accum_cov.cereal: 2420 x 2420 (symmetric, so the column-major payload is also row-major)
bool load_cov_cereal(const std::string &path, std::vector<float> &cov);
bool save_cov_cereal(const std::string &path, const std::vector<float> &cov);
// <cache>/spectros/<stem>: Spectrogram = Eigen::Matrix<float, 121, Dynamic>, element (b, c) at b + 121 c.  The device
// layout is bin-major [121][C]: save transposes; load returns the matrix as stored (column-major)
bool save_spectro_cereal(const std::string &path, const float *binmajor, int32_t cols);
bool load_spectro_cereal(const std::string &path, std::vector<float> &colmajor, int32_t &cols);

} // namespace hpfw
