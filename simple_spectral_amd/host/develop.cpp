#include "develop.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace ssx {
namespace {

double table_delta(const Spectrum& t) {
	return (static_cast<double>(t.high()) - static_cast<double>(t.low())) / static_cast<double>(t.samples().size() - 1);
}

// the table's knots low + k * delta, k = -1 .. n, that lie strictly inside (a, z)
void knots_inside(const Spectrum& t, double a, double z, std::vector<double>* out) {
	const double low = static_cast<double>(t.low()), delta = table_delta(t);
	const long n = static_cast<long>(t.samples().size());
	for (long k = -1; k <= n; ++k) {
		const double x = low + static_cast<double>(k) * delta;
		if (x > a && x < z) out->push_back(x);
	}
}

} // namespace

double table_at(const Spectrum& t, double lambda) {
	const std::vector<float>& s = t.samples();
	const double pos = (lambda - static_cast<double>(t.low())) / table_delta(t);
	const double base = std::floor(pos);
	const double n = static_cast<double>(s.size());
	if (!(base >= -1.0) || !(base < n)) return 0.0; // both neighbours outside the table (or lambda not a number)
	const double f = pos - base;
	const long i = static_cast<long>(base);
	auto at = [&s](long k) { return (k >= 0 && static_cast<size_t>(k) < s.size()) ? static_cast<double>(s[static_cast<size_t>(k)]) : 0.0; };
	return at(i) * (1.0 - f) + at(i + 1) * f;
}

double table_integral(const Spectrum& r, const Spectrum* g, double a, double z) {
	std::vector<double> x{ a };
	knots_inside(r, a, z, &x);
	if (g) knots_inside(*g, a, z, &x);
	x.push_back(z);
	std::sort(x.begin(), x.end());
	x.erase(std::unique(x.begin(), x.end()), x.end());
	auto F = [&](double lambda) { return g ? table_at(r, lambda) * table_at(*g, lambda) : table_at(r, lambda); };
	double total = 0.0;
	for (size_t i = 0; i + 1 < x.size(); ++i) {
		const double p = x[i], q = x[i + 1];
		total += ((q - p) / 6.0) * ((F(p) + 4.0 * F(0.5 * (p + q))) + F(q));
	}
	return total;
}

double bin_edge(uint32_t b, uint32_t bins, float lambda_min, float lambda_step) {
	return static_cast<double>(lambda_min) + static_cast<double>(b) * (static_cast<double>(lambda_step) / static_cast<double>(bins / 4u));
}

std::vector<double> develop_weights(const std::vector<Spectrum>& responses, const Spectrum* filter, const double* gain, const float* xyz_to_lrgb,
                                    uint32_t bins, float lambda_min, float lambda_step) {
	const size_t C = responses.size();
	if (bins < 4 || bins > 64 || bins % 4) throw HostError{ -2, "develop weights: the bin count must be a multiple of 4 up to 64" };
	if (C < 1 || C > 16) throw HostError{ -2, "develop weights: 1 to 16 response curves" };
	if (xyz_to_lrgb && C != 3) throw HostError{ -2, "develop weights: the lrgb space needs exactly three (X, Y, Z) response curves" };
	std::vector<double> w(C * bins);
	for (uint32_t b = 0; b < bins; ++b) {
		const double a = bin_edge(b, bins, lambda_min, lambda_step), z = bin_edge(b + 1, bins, lambda_min, lambda_step);
		for (size_t c = 0; c < C; ++c) {
			const double integral = table_integral(responses[c], filter, a, z);
			w[c * bins + b] = gain ? gain[b] * integral : integral;
		}
		if (xyz_to_lrgb) {
			const double X = w[b], Y = w[bins + b], Z = w[2 * bins + b];
			for (size_t r = 0; r < 3; ++r) // column-major m[c][r], as ColorData::ciexyz_to_lrgb multiplies
				w[r * bins + b] = (static_cast<double>(xyz_to_lrgb[r]) * X + static_cast<double>(xyz_to_lrgb[3 + r]) * Y) + static_cast<double>(xyz_to_lrgb[6 + r]) * Z;
		}
	}
	return w;
}

std::vector<double> relight_gain(const Spectrum& from, const Spectrum& to, uint32_t bins, float lambda_min, float lambda_step) {
	if (bins < 4 || bins > 64 || bins % 4) throw HostError{ -2, "relight gain: the bin count must be a multiple of 4 up to 64" };
	std::vector<double> g(bins);
	for (uint32_t b = 0; b < bins; ++b) {
		const double a = bin_edge(b, bins, lambda_min, lambda_step), z = bin_edge(b + 1, bins, lambda_min, lambda_step);
		const double den = table_integral(from, nullptr, a, z);
		g[b] = den == 0.0 ? 0.0 : table_integral(to, nullptr, a, z) / den;
	}
	return g;
}

void develop_white(const float* weights, uint32_t bins, float lambda_min, float lambda_step, const Spectrum* illuminant, double out[3]) {
	if (bins < 4 || bins > 64 || bins % 4) throw HostError{ -2, "develop white: the bin count must be a multiple of 4 up to 64" };
	out[0] = out[1] = out[2] = 0.0;
	for (uint32_t b = 0; b < bins; ++b) {
		const double a = bin_edge(b, bins, lambda_min, lambda_step), z = bin_edge(b + 1, bins, lambda_min, lambda_step);
		const double mean = illuminant ? table_integral(*illuminant, nullptr, a, z) / (z - a) : 1.0;
		for (size_t c = 0; c < 3; ++c) out[c] = out[c] + static_cast<double>(weights[c * bins + b]) * mean;
	}
}

uint32_t emitter_spectrum(const ssx_scene_desc& d) {
	auto emissive = [&d](const ssx_spectrum& s) {
		for (uint32_t i = 0; i < s.n; ++i) if (d.samples[s.offset + i] != 0.0f) return true;
		return false;
	};
	bool have = false;
	uint32_t first = 0, pivot = 0;
	for (uint32_t m = 0; m < d.n_materials; ++m) {
		const uint32_t idx = d.materials[m].emission_spectrum;
		if (idx >= d.n_spectra) throw HostError{ -3, "emitter spectrum: a material names a spectrum the scene does not have" };
		const ssx_spectrum& s = d.spectra[idx];
		if (!emissive(s)) continue;
		if (!have) {
			have = true; first = idx;
			while (d.samples[s.offset + pivot] == 0.0f) ++pivot;
			continue;
		}
		const ssx_spectrum& f = d.spectra[first];
		bool same = s.n == f.n && s.low == f.low && s.high == f.high;
		// s = k * f for one k: s_i * f_pivot == f_i * s_pivot for every i (products of two binary32 values are exact in binary64)
		for (uint32_t i = 0; same && i < s.n; ++i)
			same = static_cast<double>(d.samples[s.offset + i]) * static_cast<double>(d.samples[f.offset + pivot]) ==
			       static_cast<double>(d.samples[f.offset + i]) * static_cast<double>(d.samples[s.offset + pivot]);
		if (!same) throw HostError{ -3, "the scene's emissive materials carry different emission spectra (materials' spectra " + std::to_string(first) + " and " + std::to_string(idx) +
		                                    "): relighting by a gain per bin is exact only when all emitters share one spectrum up to a scale" };
	}
	if (!have) throw HostError{ -3, "the scene has no emissive material: nothing to relight" };
	return first;
}

Spectrum load_spectrum_csv(const std::string& path) {
	const size_t slash = path.rfind('/');
	const std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
	float low = 0, step = 0, high = 0;
	const size_t dash = name.rfind('-');
	const bool csv = name.size() > 4 && name.compare(name.size() - 4, 4, ".csv") == 0;
	// the numbers are read from the name without its ".csv": %f would take the extension's dot with the last of them
	const std::string range = csv && dash != std::string::npos && dash + 1 < name.size() - 4 ? name.substr(dash + 1, name.size() - 4 - (dash + 1)) : std::string();
	int used = 0;
	if (range.empty() || std::sscanf(range.c_str(), "%f+%f+%f%n", &low, &step, &high, &used) != 3 || static_cast<size_t>(used) != range.size() || !(step > 0.0f) || !(high > low))
		throw HostError{ -2, "\"" + path + "\": a spectrum file names its range, NAME-LOW+STEP+HIGH.csv (like data/d65-300+5+780.csv)" };
	std::vector<float> column = load_spectral_data(path)[0];
	const double n = (static_cast<double>(high) - static_cast<double>(low)) / static_cast<double>(step) + 1.0;
	if (column.size() < 2 || static_cast<double>(column.size()) != n)
		throw HostError{ -3, "\"" + path + "\": " + std::to_string(column.size()) + " rows do not match the range in the file's name" };
	return Spectrum(std::move(column), low, high);
}

} // namespace ssx
