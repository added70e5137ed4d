// Host build of csrc/ss_asin.h (tests/test_ocsort_cpu.py): float64 values on stdin -> ss_asin of each on stdout, raw bytes.
#include <cstdio>
#include <vector>

#include "../strongsort_yolo_amd/csrc/ss_asin.h"

int main()
{
    std::vector<double> v;
    double x;
    while (fread(&x, sizeof x, 1, stdin) == 1) v.push_back(x);
    for (double& e : v) e = ss_asin(e);
    return fwrite(v.data(), sizeof(double), v.size(), stdout) == v.size() ? 0 : 1;
}
