# Convenience targets (the driver uses __graft_entry__.py, pytest and bench.py directly).
.PHONY: build test-cpu test-cpu-asan test-gpu bench smoke clean

build:
	python -c "import __graft_entry__ as g; g.build()"

test-cpu: build
	python -m pytest tests -q -m "not gpu"

# One sanitizer pass over everything of this repository that runs on the CPU (GPU AddressSanitizer is not available on
# the pool): the oracle (oracle/_asan/libhh_oracle.so, loaded into a python that has libasan preloaded) driven by its
# own pin and property tests, and the host builds of the device headers — hh_math.h, hh_bessel.h (g++), hh_rng.h
# (hipcc, host side only) — each under AddressSanitizer + UBSan.  detect_leaks=0: the interpreter's own allocations.
# Then the Bates step composed from hh_qe.h and hh_jump.h (tests/c/bates_host_check.cpp): a program of its own, built
# with -fsanitize=address,undefined by its test and run as a program — nothing preloaded, nothing loaded into python.
# The same for the local-volatility table and for the Sobol' expansion, point rule and bridge table of hh_sobol.h
# (tests/c/sobol_host_check.cpp), and for the gamma sampler of hh_vg.h (tests/c/vg_host_check.cpp).
ASAN_RT := $(shell gcc -print-file-name=libasan.so)
test-cpu-asan:
	$(MAKE) -C oracle -s asan
	HH_SANITIZE=1 LD_PRELOAD=$(ASAN_RT) ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	  python -m pytest tests/test_oracle_pins.py tests/test_properties.py tests/test_math_host.py tests/test_bessel_host.py \
	  tests/test_rng_host.py tests/test_scratch_layout_host.py -q -m "not gpu" -p no:cacheprovider
	python -m pytest tests/test_bates_host.py -q -p no:cacheprovider -k step_host_program
	python -m pytest tests/test_localvol_host.py -q -p no:cacheprovider -k host_program
	python -m pytest tests/test_sobol_host.py -q -p no:cacheprovider -k host_program
	python -m pytest tests/test_vg_host.py -q -p no:cacheprovider -k host_program

test-gpu: build
	python -m pytest tests -q -m gpu

smoke: build
	python -c "import __graft_entry__ as g; g.smoke()"

bench: build
	python bench.py

clean:
	rm -f hedgehog.jl_amd/lib/*.so oracle/*.so tools/ubench/valu_rates
	rm -rf hedgehog.jl_amd/lib/variants
