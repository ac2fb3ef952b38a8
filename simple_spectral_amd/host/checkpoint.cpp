#include "checkpoint.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>

namespace ssx {

namespace {
const char kMagic[8] = { 'S', 'S', 'X', 'C', 'K', 'P', 'T', '1' };
const char kMagicSpectral[8] = { 'S', 'S', 'X', 'C', 'K', 'P', 'T', '2' }; // ... with the wavelength bins behind s2
const char kMagicMoments[8] = { 'S', 'S', 'X', 'C', 'K', 'P', 'T', '3' };  // ... and their second moments behind the counts
bool valid_bins(uint32_t bins) { return bins >= 4u && bins <= 64u && bins % 4u == 0u; }

// 64-bit checksum: eight bytes at a time through the splitmix64 finaliser, the length first
uint64_t mix(uint64_t h, uint64_t w) {
	uint64_t z = (h ^ w) + 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
uint64_t checksum(const uint8_t* p, size_t n) {
	uint64_t h = mix(0x535358434B505431ull, (uint64_t)n);
	for (; n >= 8; n -= 8, p += 8) { uint64_t w; std::memcpy(&w, p, 8); h = mix(h, w); }
	if (n) { uint64_t w = 0; std::memcpy(&w, p, n); h = mix(h, w); }
	return h;
}

void put(std::vector<uint8_t>& b, const void* p, size_t n) { const uint8_t* q = static_cast<const uint8_t*>(p); b.insert(b.end(), q, q + n); }
void put_u32(std::vector<uint8_t>& b, uint32_t v) { put(b, &v, 4); }

struct Reader {
	const std::vector<uint8_t>& b; size_t at = 0; const std::string& path;
	void take(void* out, size_t n) {
		if (n > b.size() - at) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is truncated" };
		std::memcpy(out, b.data() + at, n); at += n;
	}
	uint32_t u32() { uint32_t v; take(&v, 4); return v; }
	std::string text() {
		const uint32_t n = u32();
		if (n > b.size() - at) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is truncated" };
		std::string s(reinterpret_cast<const char*>(b.data() + at), n); at += n;
		return s;
	}
};
} // namespace

void checkpoint_save(const std::string& path, const Checkpoint& c) {
	const size_t pixels = (size_t)c.info.width * c.info.height;
	if (c.info.struct_size != sizeof(ssx_sums_info_t) || pixels == 0 || c.sums.size() != pixels * 4 || (!c.s2.empty() && c.s2.size() != pixels))
		throw HostError{ SSX_ERR_ARG, "checkpoint_save: the arrays do not have the size the description names" };
	const bool spectral = c.spectral.bins != 0u;
	if (!spectral && (!c.spectral_sums.empty() || !c.spectral_counts.empty())) throw HostError{ SSX_ERR_ARG, "checkpoint_save: wavelength bins without their description" };
	if (spectral && (c.spectral.struct_size != sizeof(ssx_spectral_info_t) || !valid_bins(c.spectral.bins) || c.spectral.width != c.info.width || c.spectral.height != c.info.height ||
	                 c.spectral.done_spp != c.info.done_spp || c.spectral_sums.size() != pixels * c.spectral.bins || c.spectral_counts.size() != pixels * (c.spectral.bins / 4u)))
		throw HostError{ SSX_ERR_ARG, "checkpoint_save: the wavelength bins do not belong to these sums (size, sample count, or a bin count that is no multiple of 4 in 4..64)" };
	const bool moments = !c.moments.empty();
	if (moments && !spectral) throw HostError{ SSX_ERR_ARG, "checkpoint_save: second moments without the wavelength bins they belong to" };
	if (moments && c.moments.size() != c.spectral_sums.size()) throw HostError{ SSX_ERR_ARG, "checkpoint_save: the second moments do not have the size of the wavelength bins' sums" };
	std::vector<uint8_t> b;
	b.reserve(160 + c.scene_name.size() + c.options_text.size() + (c.sums.size() + c.s2.size() + c.spectral_sums.size() + c.moments.size()) * 8 + c.spectral_counts.size() * 4);
	put(b, moments ? kMagicMoments : spectral ? kMagicSpectral : kMagic, 8);
	put_u32(b, (uint32_t)sizeof c.info); put(b, &c.info, sizeof c.info);
	put_u32(b, (uint32_t)c.scene_name.size()); put(b, c.scene_name.data(), c.scene_name.size());
	put_u32(b, (uint32_t)c.options_text.size()); put(b, c.options_text.data(), c.options_text.size());
	put_u32(b, c.s2.empty() ? 0u : 1u); put_u32(b, 0u);
	put(b, c.sums.data(), c.sums.size() * 8);
	put(b, c.s2.data(), c.s2.size() * 8);
	if (spectral) {
		put_u32(b, (uint32_t)sizeof c.spectral); put(b, &c.spectral, sizeof c.spectral);
		put(b, c.spectral_sums.data(), c.spectral_sums.size() * 8);
		put(b, c.spectral_counts.data(), c.spectral_counts.size() * 4);
		put(b, c.moments.data(), c.moments.size() * 8);
	}
	const uint64_t sum = checksum(b.data(), b.size());
	put(b, &sum, 8);
	// written next to the target and renamed over it: an interrupted save leaves the previous checkpoint whole
	const std::string tmp = path + ".part";
	{
		std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
		f.write(reinterpret_cast<const char*>(b.data()), (std::streamsize)b.size());
		f.flush();
		if (!f.good()) { std::remove(tmp.c_str()); throw HostError{ SSX_ERR_DATA, "Could not write checkpoint \"" + path + "\"" }; }
	}
	if (std::rename(tmp.c_str(), path.c_str()) != 0) { std::remove(tmp.c_str()); throw HostError{ SSX_ERR_DATA, "Could not write checkpoint \"" + path + "\"" }; }
}

Checkpoint checkpoint_load(const std::string& path) {
	std::vector<uint8_t> b;
	{
		std::ifstream f(path, std::ios::binary);
		if (!f.good()) throw HostError{ SSX_ERR_DATA, "Could not open checkpoint \"" + path + "\"" };
		b.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
	}
	const bool moments = b.size() >= 8 && std::memcmp(b.data(), kMagicMoments, 8) == 0;
	const bool spectral = moments || (b.size() >= 8 && std::memcmp(b.data(), kMagicSpectral, 8) == 0);
	if (!spectral && (b.size() < 8 || std::memcmp(b.data(), kMagic, 8) != 0)) throw HostError{ SSX_ERR_DATA, "\"" + path + "\" is not a checkpoint (magic SSXCKPT1, SSXCKPT2 or SSXCKPT3 missing)" };
	Reader r{ b, 8, path };
	Checkpoint c;
	if (r.u32() != sizeof c.info) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\": description of another size" };
	r.take(&c.info, sizeof c.info);
	c.scene_name = r.text();
	c.options_text = r.text();
	const uint32_t has_s2 = r.u32();
	(void)r.u32();
	const uint64_t pixels = (uint64_t)c.info.width * c.info.height;
	if (c.info.struct_size != sizeof c.info || pixels == 0 || pixels > (1ull << 28) || has_s2 > 1u) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is corrupt (description)" };
	const uint64_t payload = pixels * (has_s2 ? 5u : 4u) * 8u;
	uint64_t spectral_payload = 0; // the section's bytes; its header lies behind the pixel sums
	if (spectral) {
		if (b.size() - r.at < payload + 4u + sizeof c.spectral) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is truncated" };
		Reader h{ b, r.at + (size_t)payload, path };
		if (h.u32() != sizeof c.spectral) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\": spectral description of another size" };
		h.take(&c.spectral, sizeof c.spectral);
		if (c.spectral.struct_size != sizeof c.spectral || !valid_bins(c.spectral.bins) || c.spectral.width != c.info.width || c.spectral.height != c.info.height || c.spectral.done_spp != c.info.done_spp)
			throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is corrupt (spectral description: a bin count outside 4..64, or a size or sample count other than the pixel sums')" };
		spectral_payload = 4u + sizeof c.spectral + pixels * c.spectral.bins * 8u + pixels * (c.spectral.bins / 4u) * 4u;
		if (moments) spectral_payload += pixels * c.spectral.bins * 8u; // (the magic decides: the other magic on this file, or this one on the shorter, fails the length)
	}
	if (b.size() - r.at < payload + spectral_payload + 8u) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is truncated" };
	if (b.size() - r.at != payload + spectral_payload + 8u) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is corrupt (length)" };
	uint64_t stored;
	std::memcpy(&stored, b.data() + b.size() - 8, 8);
	if (stored != checksum(b.data(), b.size() - 8)) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is corrupt (checksum)" };
	c.sums.resize(pixels * 4);
	r.take(c.sums.data(), c.sums.size() * 8);
	if (has_s2) { c.s2.resize(pixels); r.take(c.s2.data(), c.s2.size() * 8); }
	if (spectral) {
		r.at += 4u + sizeof c.spectral; // (read and checked above)
		c.spectral_sums.resize(pixels * c.spectral.bins);
		r.take(c.spectral_sums.data(), c.spectral_sums.size() * 8);
		c.spectral_counts.resize(pixels * (c.spectral.bins / 4u));
		r.take(c.spectral_counts.data(), c.spectral_counts.size() * 4);
		if (moments) { c.moments.resize(pixels * c.spectral.bins); r.take(c.moments.data(), c.moments.size() * 8); }
	}
	return c;
}

bool sums_owner(const ssx_sums_info_t& info, size_t i, size_t j) {
	const size_t stride = info.tile_stride ? info.tile_stride : 1u;
	return shared_tile(info.width, info.tile_skew, i, j) % stride == info.tile_first;
}

void sums_merge(double* dst, double* dst_s2, const double* src, const double* src_s2, const ssx_sums_info_t& src_info) {
	merge_owned(dst, src, 4, src_info);
	if (dst_s2 && src_s2) merge_owned(dst_s2, src_s2, 1, src_info);
}

void spectral_merge(double* dst_sums, uint32_t* dst_counts, const double* src_sums, const uint32_t* src_counts, size_t bins, const ssx_sums_info_t& src_info) {
	if (dst_sums && src_sums) merge_owned(dst_sums, src_sums, bins, src_info);
	if (dst_counts && src_counts) merge_owned(dst_counts, src_counts, bins / 4u, src_info);
}

void moments_merge(double* dst_q, const double* src_q, size_t bins, const ssx_sums_info_t& src_info) { merge_owned(dst_q, src_q, bins, src_info); }

} // namespace ssx
