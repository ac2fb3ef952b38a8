// develop.hpp -- the host part of "Developing the spectral bins" (include/ssx.h): the weight matrix of an observer, a sensor or a filter over the wavelength
// bins, built in binary64 by exact piecewise integration of the tabulated spectra, the per-bin gain of a relighting, and the test a relighting needs (one
// emission spectrum in the scene, up to a scale).  Everything here is stated operation by operation in the header; tests/develop_ref.py restates it.
#pragma once
#include "../../include/ssx.h"
#include "spectrum.hpp"

#include <cstdint>
#include <string>
#include <vector>

namespace ssx {

// T(lambda) of include/ssx.h: the table as Spectrum::linear samples it, in binary64 -- linear to zero over one step beyond either end, zero beyond
double table_at(const Spectrum& t, double lambda);
// integral over [a, z] of r * g (g == nullptr: of r): Simpson's rule on every piece between the tables' knots, pieces added in ascending order
double table_integral(const Spectrum& r, const Spectrum* g, double a, double z);
// lower edge of bin b of B: (double)lambda_min + b * ((double)lambda_step / (B / 4))
double bin_edge(uint32_t b, uint32_t bins, float lambda_min, float lambda_step);

// [C][B] in binary64, before the final rounding: gain[b] * integral of r_c * g over bin b; with xyz_to_lrgb (9 floats, column-major; then C must be 3) the
// matrix applied to the three rows.  gain == nullptr: 1.
std::vector<double> develop_weights(const std::vector<Spectrum>& responses, const Spectrum* filter, const double* gain, const float* xyz_to_lrgb,
                                    uint32_t bins, float lambda_min, float lambda_step);
// [B]: integral of `to` over the bin / integral of `from`, 0 where the latter is 0
std::vector<double> relight_gain(const Spectrum& from, const Spectrum& to, uint32_t bins, float lambda_min, float lambda_step);
// The development of an illuminant's per-bin mean, the reference white of a colour difference (ssx.h "Colour difference of two developments"): out[c] = sum over b
// of (double)weights[c][b] * (integral of the illuminant over bin b / the bin's width), binary64, ascending b from 0.0; illuminant NULL: equal energy, mean 1.
void develop_white(const float* weights, uint32_t bins, float lambda_min, float lambda_step, const Spectrum* illuminant, double out[3]);

// The emission spectrum all emissive materials of the scene share up to a scale: its index in desc.spectra.  Throws HostError (-3) when there is no emissive
// material or when two of them carry different spectra -- a relighting by a gain per bin is then not exact.
uint32_t emitter_spectrum(const ssx_scene_desc& desc);

// One column of a file in the format of data/*.csv; its range is in the file's name: NAME-LOW+STEP+HIGH.csv (e.g. d65-300+5+780.csv).
Spectrum load_spectrum_csv(const std::string& path);

} // namespace ssx
