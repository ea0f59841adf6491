// Prints svo_lod::lod_floor(coef, bias, fine_depth) for every argument triple, one value per line
// (tests/test_lod.py).  Includes nothing of the project but that header.
#include <cstdio>
#include <cstdlib>

#include "svo_lod.h"

int main(int argc, char **argv) {
    for (int i = 1; i + 2 < argc; i += 3)
        std::printf("%.9g\n", (double)svo_lod::lod_floor(std::atof(argv[i]), std::atof(argv[i + 1]), std::atoi(argv[i + 2])));
    return 0;
}
