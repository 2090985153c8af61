// gk:52-59 on host cores: the host engine's per-value stats step (gk_cpu.cpp,
// every stream).
//
// Compiled with -ffp-contract=off and without fast-math (cpu/Makefile): the
// three roundings of gk:54 stay three IEEE roundings, so the results are the
// reference's bit for bit.
#pragma once
#include <cstdint>

// one value (gk:52-59)
inline void gk_host_stat_step(int64_t& n, double& sum, double& avg, double& mn, double& mx, double v) {
  n += 1;
  sum += v;
  avg += (v - avg) * (1.0 / (double)n);
  if (v < mn) mn = v;  // strict: the first occurrence (and a NaN never) wins
  if (v > mx) mx = v;
}
