// median_check.cpp — algorithm::computeMedian(const Eigen::VectorXd&) (src/algorithm.cpp:813-832) with the real
// libstdc++ std::nth_element, on a vector of doubles read from a binary file: prints vec[mid - 1], vec[mid] as the
// reference reads them after the call (odd length: vec[mid] twice) and the median, as hex floats.  Built and run by
// tests/two_view_ref.py: the checker of svo_two_view_init's median_depth for even counts, where vec[mid - 1] is
// whatever introselect leaves there (no GPU needed).
#include <algorithm>
#include <cstdio>
#include <limits>
#include <vector>

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> vec;
    double buf[512];
    size_t k;
    while ((k = std::fread(buf, sizeof(double), 512, f)) > 0) vec.insert(vec.end(), buf, buf + k);
    std::fclose(f);
    const auto middleSize = vec.size() / 2;
    std::nth_element(vec.begin(), vec.begin() + middleSize, vec.end());
    double lo, hi, median;
    if (vec.size() == 0) {
        lo = hi = median = std::numeric_limits<double>::quiet_NaN();
    } else if (vec.size() % 2 != 0) {  // Odd
        lo = hi = median = vec[middleSize];
    } else {  // Even
        lo = vec[middleSize - 1];
        hi = vec[middleSize];
        median = (vec[middleSize - 1] + vec[middleSize]) / 2.0;
    }
    std::printf("%a %a %a\n", lo, hi, median);
    return 0;
}
