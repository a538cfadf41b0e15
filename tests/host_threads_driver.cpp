// host_threads_driver.cpp -- csrc/host_threads.h on the CPU, under sanitizers (tests/test_host_threads_host.py builds and
// runs it): the ranges of for_ranges, a job that throws, a process that is out of threads, the worker count.
// With -DSLAMPP_HOST_THREADS_TEST_FAIL_AFTER=k the header's thread start throws std::system_error(EAGAIN) from the k-th
// start of a fork-join on; everything below must hold there as well.
#include "host_threads.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <new>

using namespace slampp;

static int n_failed = 0;
#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++ n_failed; } } while(0)

// every worker once, worker t on the formula's range, the ranges end to end over [n_begin, n_begin + n)
static void Test_Ranges()
{
	const int workers[] = {1, 2, 8};
	const int64_t begins[] = {0, 7};
	for(int n_workers : workers) {
		const int64_t sizes[] = {0, 1, n_workers - 1, n_workers, n_workers + 1, 1000003};
		for(int64_t n_begin : begins) {
			for(int64_t n : sizes) {
				struct TSeen { int n_calls = 0; int64_t n_first = -1, n_last = -1; };
				std::vector<TSeen> seen;
				seen.resize(size_t(n_workers)); // (a slot per worker: nothing shared)
				std::atomic<int> n_out_of_range(0);
				for_ranges(n_begin, n_begin + n, n_workers, [&](int t, int64_t n_first, int64_t n_last) {
					if(t < 0 || t >= n_workers) {
						++ n_out_of_range;
						return;
					}
					++ seen[size_t(t)].n_calls;
					seen[size_t(t)].n_first = n_first;
					seen[size_t(t)].n_last = n_last;
				});
				CHECK(!n_out_of_range.load());
				int64_t n_at = n_begin;
				for(int t = 0; t < n_workers; ++ t) {
					CHECK(seen[size_t(t)].n_calls == 1);
					CHECK(seen[size_t(t)].n_first == n_begin + n * t / n_workers);
					CHECK(seen[size_t(t)].n_last == n_begin + n * (t + 1) / n_workers);
					CHECK(seen[size_t(t)].n_first == n_at && seen[size_t(t)].n_last >= n_at); // no gap, no overlap
					n_at = seen[size_t(t)].n_last;
				}
				CHECK(n_at == n_begin + n);
			}
		}
	}
}

// a job that throws: the caller gets the exception, after every other job has run to its end
static void Test_Throwing_Job()
{
	const int n_jobs = 8;
	const int throwers[] = {0, n_jobs / 2, n_jobs - 1};
	for(int n_thrower : throwers) {
		std::vector<std::atomic<int> > done(n_jobs);
		for(int t = 0; t < n_jobs; ++ t)
			done[size_t(t)].store(0);
		bool b_caught = false;
		int n_done_at_catch = 0;
		try {
			run_on_threads(n_jobs, [&](int t) {
				if(t == n_thrower)
					throw std::bad_alloc();
				volatile double f_sum = 0;
				for(int i = 0; i < 200000; ++ i) // (still at work when the thrower is long gone)
					f_sum = f_sum + i;
				++ done[size_t(t)];
			});
		} catch(std::bad_alloc&) {
			b_caught = true;
			for(int t = 0; t < n_jobs; ++ t)
				n_done_at_catch += done[size_t(t)].load();
		}
		CHECK(b_caught);
		CHECK(n_done_at_catch == n_jobs - 1);
		for(int t = 0; t < n_jobs; ++ t)
			CHECK(done[size_t(t)].load() == (t != n_thrower));
	}
	{ // several throw: one exception comes out, the first that was caught
		bool b_caught = false;
		try {
			for_ranges(0, 800, 8, [&](int t, int64_t, int64_t) {
				if(t & 1)
					throw std::bad_alloc();
			});
		} catch(std::bad_alloc&) {
			b_caught = true;
		}
		CHECK(b_caught);
	}
	run_on_threads(0, [&](int) { CHECK(false); }); // no job: nothing runs
}

// every job exactly once and nothing thrown, however many threads could be started
static void Test_Every_Job_Once()
{
	const int n_jobs = 8;
	std::vector<std::atomic<int> > ran(n_jobs);
	for(int t = 0; t < n_jobs; ++ t)
		ran[size_t(t)].store(0);
	std::atomic<int> n_on_caller(0);
	const std::thread::id t_caller = std::this_thread::get_id();
	bool b_threw = false;
	try {
		run_on_threads(n_jobs, [&](int t) {
			++ ran[size_t(t)];
			if(std::this_thread::get_id() == t_caller)
				++ n_on_caller;
		});
	} catch(...) {
		b_threw = true;
	}
	CHECK(!b_threw);
	for(int t = 0; t < n_jobs; ++ t)
		CHECK(ran[size_t(t)].load() == 1);
#ifdef SLAMPP_HOST_THREADS_TEST_FAIL_AFTER
	CHECK(n_on_caller.load() == n_jobs - std::min(SLAMPP_HOST_THREADS_TEST_FAIL_AFTER, n_jobs - 1)); // job 0 and the ones no thread was to be had for
#else
	CHECK(n_on_caller.load() == 1);
#endif
}

// what the passes used to spell out, each for itself
static int n_Pasted_Expression(int64_t n, int64_t n_grain, int n_max)
{
	return int(std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_max, std::max(1u, std::thread::hardware_concurrency())), n / n_grain)));
}

static void Test_Thread_Count()
{
	const struct { int64_t n, n_grain; int n_max; } table[] = {
		{0, 65536, 8}, {1, 65536, 8}, {65535, 65536, 8}, {65536, 65536, 8}, {131071, 65536, 8}, {131072, 65536, 8},
		{524287, 65536, 8}, {524288, 65536, 8}, {2000000, 65536, 8}, {int64_t(1) << 40, 65536, 8},
		{32767, 32768, 8}, {100000, 32768, 8}, {4096, 2048, 8}, {2047, 2048, 8}, {100000, 16384, 8},
		{65536, 16384, 4}, {65535, 16384, 4}, {16383, 16384, 4}, {1 << 20, 4096, 4}, {1 << 20, 512, 4}, {100, 32, 4},
		{1 << 20, 65536, 1}, {1 << 20, 65536, 0}, {1 << 20, 8, 8}
	};
	for(const auto &r : table) {
		CHECK(host_thread_count(r.n, r.n_grain, r.n_max) == n_Pasted_Expression(r.n, r.n_grain, r.n_max));
		if(r.n < r.n_grain)
			CHECK(host_thread_count(r.n, r.n_grain, r.n_max) == 1);
	}
	CHECK(host_thread_count(1 << 20, 65536) == host_thread_count(1 << 20, 65536, 8)); // the default: eight
	// the development knobs (plan.h): nothing without SLAMPP_HIP_DEV=1
	setenv("SLAMPP_HIP_DEV_HOST_THREAD_GRAIN", "256", 1);
	setenv("SLAMPP_HIP_DEV_SETUP_THREADS", "2", 1);
	dev_knobs_refresh();
	CHECK(host_thread_count(4000, 65536) == 1);
	setenv("SLAMPP_HIP_DEV", "1", 1);
	dev_knobs_refresh();
	CHECK(host_thread_count(4000, 65536) == n_Pasted_Expression(4000, 256, 2));
	unsetenv("SLAMPP_HIP_DEV_SETUP_THREADS");
	CHECK(host_thread_count(4000, 65536) == n_Pasted_Expression(4000, 256, 8));
	CHECK(host_thread_count(255, 65536) == 1);
	unsetenv("SLAMPP_HIP_DEV_HOST_THREAD_GRAIN");
	CHECK(host_thread_count(4000, 65536) == 1);
	unsetenv("SLAMPP_HIP_DEV");
	dev_knobs_refresh();
}

int main()
{
	unsetenv("SLAMPP_HIP_DEV");
	dev_knobs_refresh();
	Test_Ranges();
	Test_Throwing_Job();
	Test_Every_Job_Once();
	Test_Thread_Count();
	{ // the guard joins what it holds
		std::atomic<int> n_ran(0);
		{
			CJoinedThread t_guard;
			t_guard.t = std::thread([&]() { ++ n_ran; });
		}
		CHECK(n_ran.load() == 1);
	}
	if(n_failed) {
		fprintf(stderr, "host_threads_driver: %d checks failed\n", n_failed);
		return 1;
	}
	printf("host_threads_driver: ok\n");
	return 0;
}
