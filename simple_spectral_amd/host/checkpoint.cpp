#include "checkpoint.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>

namespace ssx {

namespace {
const char kMagic[8] = { 'S', 'S', 'X', 'C', 'K', 'P', 'T', '1' };

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
	std::vector<uint8_t> b;
	b.reserve(128 + c.scene_name.size() + c.options_text.size() + (c.sums.size() + c.s2.size()) * 8);
	put(b, kMagic, 8);
	put_u32(b, (uint32_t)sizeof c.info); put(b, &c.info, sizeof c.info);
	put_u32(b, (uint32_t)c.scene_name.size()); put(b, c.scene_name.data(), c.scene_name.size());
	put_u32(b, (uint32_t)c.options_text.size()); put(b, c.options_text.data(), c.options_text.size());
	put_u32(b, c.s2.empty() ? 0u : 1u); put_u32(b, 0u);
	put(b, c.sums.data(), c.sums.size() * 8);
	put(b, c.s2.data(), c.s2.size() * 8);
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
	if (b.size() < 8 || std::memcmp(b.data(), kMagic, 8) != 0) throw HostError{ SSX_ERR_DATA, "\"" + path + "\" is not a checkpoint (magic SSXCKPT1 missing)" };
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
	if (b.size() - r.at < payload + 8u) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is truncated" };
	if (b.size() - r.at != payload + 8u) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is corrupt (length)" };
	uint64_t stored;
	std::memcpy(&stored, b.data() + b.size() - 8, 8);
	if (stored != checksum(b.data(), b.size() - 8)) throw HostError{ SSX_ERR_DATA, "Checkpoint \"" + path + "\" is corrupt (checksum)" };
	c.sums.resize(pixels * 4);
	r.take(c.sums.data(), c.sums.size() * 8);
	if (has_s2) { c.s2.resize(pixels); r.take(c.s2.data(), c.s2.size() * 8); }
	return c;
}

bool sums_owner(const ssx_sums_info_t& info, size_t i, size_t j) {
	const size_t stride = info.tile_stride ? info.tile_stride : 1u;
	return shared_tile(info.width, info.tile_skew, i, j) % stride == info.tile_first;
}

void sums_merge(double* dst, double* dst_s2, const double* src, const double* src_s2, const ssx_sums_info_t& src_info) {
	for (size_t j = 0; j < src_info.height; ++j) for (size_t i = 0; i < src_info.width; ++i) {
		if (!sums_owner(src_info, i, j)) continue;
		const size_t p = j * src_info.width + i;
		std::memcpy(dst + 4 * p, src + 4 * p, 4 * sizeof(double));
		if (dst_s2 && src_s2) dst_s2[p] = src_s2[p];
	}
}

} // namespace ssx
