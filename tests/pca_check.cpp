// pca_check.cpp — bvcf_pca_tri.h on its own, for tests/test_pca_cpu.py: built with the address and undefined-behaviour
// sanitizers and run directly.  Reads tridiagonal matrices from the file named by argv[1] -- per matrix a line "n k", a line of
// n diagonal entries and a line of n - 1 off-diagonal entries (hexadecimal floats; the third line is empty for n = 1) -- and
// prints per matrix a line of the k values and a line of the k * n vector components, as hexadecimal floats: the test
// compares them bit for bit with what the library's entry gives and checks them against numpy.  Every array is a heap block of
// exactly its size: a read or write past it is the sanitizer's to find.  A last line "pca_tri ok" when all went through.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bvcf_pca_tri.h"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  unsigned n = 0, k = 0;
  int fails = 0;
  while (fscanf(f, "%u %u", &n, &k) == 2) {
    double *d = (double *)malloc(sizeof(double) * (n ? n : 1));
    double *e = (double *)malloc(sizeof(double) * (n > 1 ? n - 1 : 1));
    bool ok = true;
    for (unsigned i = 0; i < n; i++) ok = ok && fscanf(f, "%la", &d[i]) == 1;
    for (unsigned i = 0; i + 1 < n; i++) ok = ok && fscanf(f, "%la", &e[i]) == 1;
    if (!ok) {
      fprintf(stderr, "FAIL: short input\n");
      return 1;
    }
    double *values = (double *)malloc(sizeof(double) * (k ? k : 1));
    double *z = (double *)malloc(sizeof(double) * ((size_t)k * n ? (size_t)k * n : 1));
    const int rc = pca_tri::solve(d, n > 1 ? e : nullptr, n, k, values, z);
    if (rc) {
      printf("refused\n\n");
    } else {
      for (unsigned a = 0; a < k; a++) printf("%a%c", values[a], a + 1 < k ? ' ' : '\n');
      for (size_t i = 0; i < (size_t)k * n; i++) printf("%a%c", z[i], i + 1 < (size_t)k * n ? ' ' : '\n');
      for (unsigned a = 1; a < k; a++)
        if (!(values[a] <= values[a - 1])) {
          fails++;
          fprintf(stderr, "FAIL: values not descending at %u\n", a);
        }
    }
    free(d);
    free(e);
    free(values);
    free(z);
  }
  fclose(f);
  if (fails) return 1;
  printf("pca_tri ok\n");
  return 0;
}
