// ssx_rccl.h -- everything RCCL: the library through dlopen, the contexts' communicators, the combine of the device framebuffers
// (ssx_reduce_rccl) and its dry run (ssx_rccl_probe).  Included by ssx_api.hip (one translation unit), behind ssx_ctx and fail().
// A process that combines by peer copies (ssx_accumulate_peer) never loads RCCL.
#pragma once

namespace {

struct RcclApi {
	void* lib = nullptr;
	int (*init_all)(void**, int, const int*) = nullptr;
	int (*group_start)() = nullptr;
	int (*group_end)() = nullptr;
	int (*reduce)(const void*, void*, size_t, int, int, int, void*, hipStream_t) = nullptr;
	int (*comm_destroy)(void*) = nullptr;
	const char* (*error_string)(int) = nullptr;
	uint64_t groups_made = 0;
	std::mutex mutex;
};
RcclApi& rccl_api() { static RcclApi api; return api; }
// opens RCCL once per process (caller holds rccl.mutex); false + the reason when it is not there or lacks an entry point
bool load_rccl(RcclApi& rccl, std::string* why) {
	if (rccl.lib) return true;
	// the soname first: a process that already holds an RCCL under that name (torch's) must not map a second one
	for (const char* name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so" }) if ((rccl.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
	if (!rccl.lib) { const char* e = dlerror(); *why = std::string("RCCL is not available (") + (e ? e : "dlopen failed") + ")"; return false; }
	rccl.init_all = (decltype(rccl.init_all))dlsym(rccl.lib, "ncclCommInitAll"); rccl.group_start = (decltype(rccl.group_start))dlsym(rccl.lib, "ncclGroupStart");
	rccl.group_end = (decltype(rccl.group_end))dlsym(rccl.lib, "ncclGroupEnd"); rccl.reduce = (decltype(rccl.reduce))dlsym(rccl.lib, "ncclReduce");
	rccl.comm_destroy = (decltype(rccl.comm_destroy))dlsym(rccl.lib, "ncclCommDestroy"); rccl.error_string = (decltype(rccl.error_string))dlsym(rccl.lib, "ncclGetErrorString");
	if (!rccl.init_all || !rccl.group_start || !rccl.group_end || !rccl.reduce || !rccl.comm_destroy || !rccl.error_string) { dlclose(rccl.lib); rccl.lib = nullptr; *why = "RCCL lacks an entry point"; return false; }
	return true;
}
// (caller holds rccl_api().mutex)
void drop_rccl_comm(ssx_ctx* ctx) {
	if (ctx->rccl_comm && rccl_api().comm_destroy) { (void)hipSetDevice(ctx->device); (void)rccl_api().comm_destroy(ctx->rccl_comm); }
	ctx->rccl_comm = nullptr; ctx->rccl_group = 0; ctx->rccl_rank = -1; ctx->rccl_size = 0;
}

// a device name or an error text as the inside of a JSON string: " and \ escaped, control characters dropped
std::string json_text(const std::string& s) {
	std::string out;
	for (const char c : s) {
		if (c == '"' || c == '\\') out += '\\';
		if ((unsigned char)c >= 0x20u) out += c;
	}
	return out;
}

} // namespace

extern "C" {

// The C++ host's combine over RCCL (north_star: "a final RCCL reduce over xGMI of the per-GPU framebuffer"): one communicator
// per context of this process (ncclCommInitAll), one grouped ncclReduce(sum, float) of the device framebuffers into
// ctxs[0]'s.  Every pixel is nonzero on exactly one device, so the sum is exact whatever the reduction tree.
// The communicators are created on the first combine of a group of contexts and KEPT in the contexts (ncclCommInitAll costs
// far more than the 4 MiB reduce it serves); a call with another group (other contexts, another order) replaces them, and
// ssx_destroy destroys what its context holds.
int ssx_reduce_rccl(ssx_ctx** ctxs, int n, uint32_t width, uint32_t height) {
	if (!ctxs || n <= 0 || !ctxs[0] || width == 0 || height == 0) return SSX_ERR_ARG;
	ssx_ctx* root = ctxs[0];
	RcclApi& rccl = rccl_api();
	std::lock_guard<std::mutex> load_guard(rccl.mutex); // one combine at a time per process (loading the library, and the communicators below)
	{ std::string why; if (!load_rccl(rccl, &why)) return fail(root, SSX_ERR_DEVICE, why); }
	std::vector<int> devs(n);
	for (int i = 0; i < n; ++i) {
		if (!ctxs[i] || ctxs[i]->d_out.bytes < image_bytes(width, height)) return fail(root, SSX_ERR_STATE, "ssx_reduce_rccl: a context has no rendered framebuffer of that size");
		if (ctxs[i]->rendering.load()) return fail(root, SSX_ERR_STATE, "ssx_reduce_rccl: render in progress");
		devs[i] = ctxs[i]->device;
		for (int k = 0; k < i; ++k) if (devs[k] == devs[i]) return fail(root, SSX_ERR_ARG, "ssx_reduce_rccl: two contexts on one device (RCCL wants one rank per device; use ssx_accumulate_peer)");
	}
	// the group's communicators: those the contexts hold from an earlier combine of the same group, or new ones.  A group is
	// named by the number ncclCommInitAll's call got here (rccl_group) -- the same in every context of it -- and the rank.
	bool have = root->rccl_comm != nullptr && root->rccl_group != 0;
	for (int i = 0; i < n && have; ++i) have = ctxs[i]->rccl_comm && ctxs[i]->rccl_group == root->rccl_group && ctxs[i]->rccl_rank == i && ctxs[i]->rccl_size == n;
	int rc = 0;
	if (!have) {
		for (int i = 0; i < n; ++i) drop_rccl_comm(ctxs[i]);
		std::vector<void*> comms(n, nullptr);
		rc = rccl.init_all(comms.data(), n, devs.data());
		if (rc) return fail(root, SSX_ERR_DEVICE, std::string("ncclCommInitAll: ") + rccl.error_string(rc));
		const uint64_t group = ++rccl.groups_made;
		for (int i = 0; i < n; ++i) { ctxs[i]->rccl_comm = comms[i]; ctxs[i]->rccl_group = group; ctxs[i]->rccl_rank = i; ctxs[i]->rccl_size = n; }
	}
	const size_t count = (size_t)width * height * 4u;
	rc = rccl.group_start();
	for (int i = 0; i < n && !rc; ++i) {
		if (hipSetDevice(devs[i]) != hipSuccess) { rc = -1; break; }
		rc = rccl.reduce(ctxs[i]->d_out.ptr, ctxs[i]->d_out.ptr, count, 7 /* ncclFloat */, 0 /* ncclSum */, 0, ctxs[i]->rccl_comm, ctxs[i]->stream);
	}
	const int rc_end = rccl.group_end();
	if (!rc) rc = rc_end;
	for (int i = 0; i < n; ++i) { (void)hipSetDevice(devs[i]); (void)hipStreamSynchronize(ctxs[i]->stream); }
	(void)hipSetDevice(root->device);
	if (rc) {
		for (int i = 0; i < n; ++i) drop_rccl_comm(ctxs[i]); // (a failed collective leaves the communicators in an unknown state)
		return fail(root, SSX_ERR_DEVICE, std::string("ncclReduce: ") + (rc > 0 ? rccl.error_string(rc) : "hipSetDevice failed"));
	}
	return SSX_OK;
}

// A dry run of the combine above on whatever this process can see (the first real multi-GPU run should be boring):
// every visible device gets a communicator (ncclCommInitAll), peer access is looked up pair by pair, one grouped ncclReduce of a
// 4 MiB float buffer per device (rank i holds i + 1 in every element) goes to device 0 and is checked there -- and whatever it finds
// is REPORTED (JSON text), not failed on: a missing library, one device only, a pair without peer access, an error code.  Returns the
// number of devices the reduce went through correctly (0 when it did not happen), or SSX_ERR_ARG.  No context needed; communicators
// and buffers are released again.
int ssx_rccl_probe(char* report, size_t report_size) {
	if (!report || report_size < 64) return SSX_ERR_ARG;
	std::string out = "{";
	auto finish = [&](int n_ok) { out += fmt("\"devices_reduced_ok\": %d}", n_ok); snprintf(report, report_size, "%s", out.c_str()); return n_ok; };
	int n = 0, before = 0;
	(void)hipGetDevice(&before);
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); out += "\"error\": \"no HIP device\", "; return finish(0); }
	out += fmt("\"visible_devices\": %d, \"devices\": [", n);
	for (int i = 0; i < n; ++i) {
		hipDeviceProp_t prop = {}; size_t free_b = 0, total_b = 0;
		const hipError_t e = hipGetDeviceProperties(&prop, i);
		(void)hipSetDevice(i); (void)hipMemGetInfo(&free_b, &total_b);
		out += fmt("%s{\"index\": %d, ", i ? ", " : "", i);
		if (e != hipSuccess) { (void)hipGetLastError(); out += "\"error\": \"hipGetDeviceProperties: " + json_text(hipGetErrorString(e)) + "\", "; }
		else out += "\"name\": \"" + json_text(prop.name) + fmt("\", \"pci\": \"%04x:%02x:%02x\", ", prop.pciDomainID, prop.pciBusID, prop.pciDeviceID);
		out += fmt("\"free_bytes\": %zu, \"total_bytes\": %zu}", free_b, total_b);
	}
	out += "], \"peer_access\": [";
	int no_peer = 0;
	for (int i = 0; i < n; ++i) {
		out += i ? ", [" : "[";
		for (int k = 0; k < n; ++k) { int can = (i == k); if (i != k) (void)hipDeviceCanAccessPeer(&can, i, k); if (!can) ++no_peer; out += fmt("%s%d", k ? ", " : "", can); }
		out += "]";
	}
	out += fmt("], \"pairs_without_peer_access\": %d, ", no_peer);
	RcclApi& rccl = rccl_api();
	std::lock_guard<std::mutex> guard(rccl.mutex);
	{ std::string why; if (!load_rccl(rccl, &why)) { out += "\"rccl\": \"" + json_text(why) + "\", "; (void)hipSetDevice(before); return finish(0); } }
	std::vector<int> devs(n); for (int i = 0; i < n; ++i) devs[i] = i;
	std::vector<void*> comms(n, nullptr);
	const auto t0 = std::chrono::steady_clock::now();
	int rc = rccl.init_all(comms.data(), n, devs.data());
	out += fmt("\"ncclCommInitAll_ms\": %.1f, ", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	if (rc) { out += "\"rccl\": \"ncclCommInitAll: " + json_text(rccl.error_string(rc)) + "\", "; (void)hipSetDevice(before); return finish(0); }
	const size_t count = (size_t)1 << 20; // floats per device: the headline image's 4 MiB
	std::vector<DeviceBuffer> buf(n); std::vector<hipStream_t> st(n, nullptr);
	bool ok = true;
	for (int i = 0; i < n && ok; ++i) {
		ok = hipSetDevice(i) == hipSuccess && buf[i].reserve(count * sizeof(float)) == hipSuccess && hipStreamCreate(&st[i]) == hipSuccess;
		if (ok) { std::vector<float> h(count, (float)(i + 1)); ok = hipMemcpy(buf[i].ptr, h.data(), count * sizeof(float), hipMemcpyHostToDevice) == hipSuccess; }
	}
	int n_ok = 0;
	if (!ok) out += "\"rccl\": \"could not set up the probe buffers\", ";
	else {
		const auto t1 = std::chrono::steady_clock::now();
		rc = rccl.group_start();
		for (int i = 0; i < n && !rc; ++i) { (void)hipSetDevice(i); rc = rccl.reduce(buf[i].ptr, buf[i].ptr, count, 7 /* ncclFloat */, 0 /* ncclSum */, 0, comms[i], st[i]); }
		const int rc_end = rccl.group_end();
		if (!rc) rc = rc_end;
		for (int i = 0; i < n; ++i) { (void)hipSetDevice(i); (void)hipStreamSynchronize(st[i]); }
		out += fmt("\"reduce_4MiB_ms\": %.2f, ", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
		if (rc) out += "\"rccl\": \"ncclReduce: " + json_text(rc > 0 ? rccl.error_string(rc) : "failed") + "\", ";
		else {
			std::vector<float> h(count);
			(void)hipSetDevice(0);
			const float want = 0.5f * (float)n * (float)(n + 1);
			size_t bad = 0;
			if (hipMemcpy(h.data(), buf[0].ptr, count * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess) { for (float v : h) bad += v != want; } else bad = count;
			out += fmt("\"rccl\": \"ok\", \"reduce_elements_wrong\": %zu, ", bad);
			if (bad == 0) n_ok = n;
		}
	}
	for (int i = 0; i < n; ++i) { (void)hipSetDevice(i); if (st[i]) (void)hipStreamDestroy(st[i]); buf[i].release(); if (comms[i]) (void)rccl.comm_destroy(comms[i]); }
	(void)hipSetDevice(before);
	return finish(n_ok);
}

// communicators created so far in this process (tests: a second combine of the same contexts must not create any)
uint64_t ssx_rccl_groups_made(void) { return rccl_api().groups_made; }

} // extern "C"
