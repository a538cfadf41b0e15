// capi_util.h -- what the translation units of the C ABI share (capi.hip, capi_covariance.hip, capi_resolve.hip): the
// mapping of exceptions to status codes, and the round trip of a host entry point through its device twin
#pragma once

#include "solver.h"

namespace {

// runs f, maps exceptions to status codes, records the message
template <class F>
int guarded(slampp_hip_solver *p, F f, bool b_join_bringup = true /* false: the entry point waits for the handle's streams itself, or needs none */)
{
	if(!p)
		return SLAMPP_HIP_ERR_INVALID;
	try {
		if(b_join_bringup)
			p->Join_Bringup();
		if(hipSetDevice(p->n_device) != hipSuccess)
			throw slampp::CDeviceError("hipSetDevice failed");
		return f();
	} catch(std::bad_alloc&) {
		p->s_error = "out of memory";
		return SLAMPP_HIP_ERR_ALLOC;
	} catch(slampp::CDeviceError &e) {
		p->s_error = e.what();
		return SLAMPP_HIP_ERR_DEVICE;
	} catch(std::domain_error &e) {
		p->s_error = e.what();
		return SLAMPP_HIP_ERR_UNSUPPORTED;
	} catch(std::exception &e) {
		p->s_error = e.what();
		return SLAMPP_HIP_ERR_INVALID;
	}
}

inline int fail(slampp_hip_solver *p, int n_code, const char *p_s_msg)
{
	p->s_error = p_s_msg;
	return n_code;
}

// The second half of a host entry point, behind its checks and uploads: the device twin, the wait, the way back.  Every step
// is skipped once one has returned anything but SLAMPP_HIP_OK.
//   device(s)   calls the _device_async entry point on the handle's own arrays;
//   b_sync      the wait is slampp_hip_sync, which answers for the not-positive-definite flag; false: nothing was factored,
//               and the synchronization that ends the last step is the wait;
//   collect(s)  enqueues the device-to-host copies (inside guarded(): throws); one hipStreamSynchronize follows them.
template <class FDevice, class FCollect>
int device_round_trip(slampp_hip_solver *p, FDevice device, bool b_sync, FCollect collect)
{
	int n_result = device(*p);
	if(n_result == SLAMPP_HIP_OK && b_sync)
		n_result = slampp_hip_sync(p);
	if(n_result == SLAMPP_HIP_OK) {
		n_result = guarded(p, [&]() -> int {
			slampp_hip_solver &s = *p;
			collect(s);
			SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream));
			return SLAMPP_HIP_OK;
		});
	}
	return n_result;
}

// A whole host entry point: prepare() (inside guarded()) checks the arguments, allocates the handle's arrays and uploads;
// then the round trip above.  *p_b_handed_over (where given), set by prepare(): the call has been answered in full -- by the
// device group of a handle over several devices -- and what prepare() returned is its result.
template <class FPrepare, class FDevice, class FCollect>
int host_round_trip(slampp_hip_solver *p, FPrepare prepare, FDevice device, bool b_sync, FCollect collect,
	const bool *p_b_handed_over = 0)
{
	const int n_result = guarded(p, prepare);
	if(n_result != SLAMPP_HIP_OK || (p_b_handed_over && *p_b_handed_over))
		return n_result;
	return device_round_trip(p, device, b_sync, collect);
}

} // anonymous namespace
