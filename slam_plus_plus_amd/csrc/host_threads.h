// host_threads.h -- the fork-join of the cold path's host passes: how many worker threads a pass gets, jobs and index
// ranges side by side with every started thread joined and the first exception handed to the caller, and a guard that
// joins one thread.  Plain C++: no HIP call, nothing of the handle.  Threads that outlive the call that started them
// are not started here: those own their catch.
#pragma once
#include "plan.h"

#include <algorithm>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>
#ifdef SLAMPP_HOST_THREADS_TEST_FAIL_AFTER
#include <cerrno>
#include <system_error>
#endif

namespace slampp {

// Worker threads for a pass over n records of which a thread should get at least n_per_thread: at most n_max, no more
// than the machine has, at least one.  Development knobs (plan.h): SLAMPP_HIP_DEV_SETUP_THREADS caps n_max,
// SLAMPP_HIP_DEV_HOST_THREAD_GRAIN replaces n_per_thread (the many-worker paths at a small system).
inline int host_thread_count(int64_t n, int64_t n_per_thread, int n_max = 8)
{
	n_max = std::min(n_max, std::max(dev_knob("SLAMPP_HIP_DEV_SETUP_THREADS", n_max), 1));
	if(dev_knob_set("SLAMPP_HIP_DEV_HOST_THREAD_GRAIN"))
		n_per_thread = dev_knob("SLAMPP_HIP_DEV_HOST_THREAD_GRAIN", 0);
	return int(std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_max, std::max(1u, std::thread::hardware_concurrency())), n / std::max<int64_t>(n_per_thread, 1))));
}

// (the one place a thread of a fork-join is started)
template <class CBody>
inline void host_thread_start(std::vector<std::thread> &r_threads, CBody body, int t)
{
#ifdef SLAMPP_HOST_THREADS_TEST_FAIL_AFTER // (tests/host_threads_driver.cpp only: no more threads from this start on)
	if(int(r_threads.size()) >= SLAMPP_HOST_THREADS_TEST_FAIL_AFTER)
		throw std::system_error(EAGAIN, std::generic_category());
#endif
	r_threads.emplace_back(body, t);
}

// job(0) .. job(n_jobs - 1) side by side: job 0 on the calling thread, the others on a thread each -- on the calling
// thread as well where no more threads can be started.  Every started thread is joined on every way out; the first
// exception a job threw is rethrown after that.
template <class CJob>
void run_on_threads(int n_jobs, CJob job)
{
	if(n_jobs <= 0)
		return;
	std::vector<std::thread> threads;
	std::exception_ptr p_error;
	std::mutex t_mutex;
	auto guarded = [&](int t) {
		try {
			job(t);
		} catch(...) {
			std::lock_guard<std::mutex> t_lock(t_mutex);
			if(!p_error)
				p_error = std::current_exception();
		}
	};
	try {
		for(int t = 1; t < n_jobs; ++ t)
			host_thread_start(threads, guarded, t);
	} catch(...) { // no more threads: the rest on this one
		for(int t = int(threads.size()) + 1; t < n_jobs; ++ t)
			guarded(t);
	}
	guarded(0);
	for(size_t t = 0; t < threads.size(); ++ t)
		threads[t].join();
	if(p_error)
		std::rethrow_exception(p_error);
}

// work(t, first, last) for the n_workers ranges that tile [n_begin, n_end), side by side: worker t owns
// [n_begin + n * t / n_workers, n_begin + n * (t + 1) / n_workers) -- what a pass keeps per worker (the counters of the
// counting sorts) is laid out by t.  One worker: on the calling thread, nothing started.
template <class CWork>
void for_ranges(int64_t n_begin, int64_t n_end, int n_workers, CWork work)
{
	if(n_workers <= 1) {
		work(0, n_begin, n_end);
		return;
	}
	const int64_t n = n_end - n_begin;
	run_on_threads(n_workers, [&](int t) { work(t, n_begin + n * t / n_workers, n_begin + n * (t + 1) / n_workers); });
}

// a thread that is joined on every way out of the scope that started it
struct CJoinedThread {
	std::thread t;
	~CJoinedThread() { if(t.joinable()) t.join(); }
};

} // namespace slampp
