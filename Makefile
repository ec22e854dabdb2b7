# Convenience targets; __graft_entry__.build() performs the same hipcc / oracle builds.
HIPCC ?= /opt/rocm/bin/hipcc
CSRC  := poulpy_amd/csrc
LIB   := poulpy_amd/libpoulpy_hip.so

all: $(LIB) oracle

UNITS := $(wildcard $(CSRC)/*.hip)
HOST_UNITS := $(wildcard $(CSRC)/*.cpp)   # plain C++, no HIP (the BDD schedule compiler)
OBJS  := $(patsubst $(CSRC)/%.hip,$(CSRC)/_obj/%.o,$(UNITS)) $(patsubst $(CSRC)/%.cpp,$(CSRC)/_obj/%.o,$(HOST_UNITS))
RCCL  := -ldl   # RCCL itself is dlopen-ed at the first pz_comm_* call (api_dist.hip)

# one object per translation unit (make -j8 compiles them in parallel; launch_br.hip is the long pole, ~75 s)
$(CSRC)/_obj/%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.hpp) include/poulpy_hip.h
	@mkdir -p $(CSRC)/_obj
	cd $(CSRC) && $(HIPCC) -O3 -std=c++17 --offload-arch=gfx950 -fPIC -c $(notdir $<) -o _obj/$(notdir $@)

$(CSRC)/_obj/%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.hpp)
	@mkdir -p $(CSRC)/_obj
	$(CXX) -O2 -std=c++17 -fPIC -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=gfx950 -fPIC -shared -o $@ $(OBJS) $(RCCL)

oracle:
	$(MAKE) -s -C oracle

# C++ client of the ABI (tests/cpp/test_abi.cpp); run it on a GPU box
cpp-test: $(LIB) oracle
	g++ -O1 -std=c++17 -I include -I oracle tests/cpp/test_abi.cpp -o tests/cpp/test_abi $(LIB) oracle/_build/libpoulpy_oracle.so \
	    -Wl,-rpath,$(CURDIR)/poulpy_amd -Wl,-rpath,$(CURDIR)/oracle/_build -Wl,-rpath,/opt/rocm/lib

# register / scratch / occupancy table of every kernel
kres:
	python tools/kres.py

test-cpu:
	python -m pytest tests -x -q -m "not gpu"

# on the GPU box (through gpurun from the build container)
test-gpu:
	python -m pytest tests -x -q -m gpu

bench:
	python bench.py

# host-only check of the BDD schedule compiler under the host sanitizers (tests/test_bdd_host.py builds and runs the same program)
cpp-test-bdd:
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/test_bdd_schedule.cpp $(CSRC)/bdd_schedule.cpp -o tests/cpp/test_bdd_schedule
	tests/cpp/test_bdd_schedule

# host-only check of the level map of FheUint::pack under the host sanitizers (tests/test_fhe_uint_pack_host.py builds and runs the same program)
cpp-test-pack:
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/test_pack_levels.cpp $(CSRC)/pack_levels.cpp -o tests/cpp/test_pack_levels
	tests/cpp/test_pack_levels

# host-only check of the stage plan of the FheUint byte operations under the host sanitizers (tests/test_fhe_uint_bytes_host.py builds and runs the same program)
cpp-test-word:
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/test_word_ops.cpp $(CSRC)/word_ops.cpp -o tests/cpp/test_word_ops
	tests/cpp/test_word_ops

# host-only check of the middle-kernel and block-step form choice under the host sanitizers (tests/test_mid_forms_host.py builds and runs the same program)
cpp-test-mid:
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/test_mid_forms.cpp -o tests/cpp/test_mid_forms
	tests/cpp/test_mid_forms tests/golden/mid128_forms.txt

# host-only check of the fused tail's launch plan under the host sanitizers (tests/test_tail_plan_host.py builds and runs the same program)
cpp-test-tail:
	$(CXX) -std=c++17 -O2 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/test_tail_plan.cpp -o tests/cpp/test_tail_plan
	tests/cpp/test_tail_plan tests/golden/tail_plans.txt

# the per-coefficient walk of k_lincomb_const on the host under the host sanitizers; it reads its cases from a file that
# tests/test_ckks_lincomb_host.py writes from the oracle (that test builds and runs the same program)
tests/cpp/test_lincomb_walk: tests/cpp/test_lincomb_walk.cpp $(wildcard $(CSRC)/*.hpp)
	$(HIPCC) -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -I $(CSRC) -I include $< -o $@ -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined

# the term planner and the per-thread walk of k_glwe_sum on the host under the host sanitizers; it reads its cases from a file that
# tests/test_ckks_sum_host.py writes from the oracle (that test builds and runs the same program)
tests/cpp/test_sum_walk: tests/cpp/test_sum_walk.cpp $(wildcard $(CSRC)/*.hpp)
	$(HIPCC) -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -I $(CSRC) -I include $< -o $@ -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined

# the shared carry steps, the same-base normalization plan and its walk (znx_steps.hpp) on the host under the host sanitizers; it reads
# its cases from a file that tests/test_znx_steps_host.py writes from the oracle (that test builds and runs the same program)
tests/cpp/test_znx_steps: tests/cpp/test_znx_steps.cpp $(CSRC)/znx_steps.hpp
	$(HIPCC) -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -I $(CSRC) $< -o $@ -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined

clean:
	rm -f $(LIB) tests/cpp/test_abi tests/cpp/test_bdd_schedule tests/cpp/test_pack_levels tests/cpp/test_word_ops tests/cpp/test_mid_forms tests/cpp/test_tail_plan tests/cpp/test_lincomb_walk tests/cpp/test_sum_walk tests/cpp/test_znx_steps
	rm -rf $(CSRC)/_obj
	rm -rf oracle/_build

.PHONY: all oracle cpp-test cpp-test-bdd cpp-test-pack cpp-test-word cpp-test-mid cpp-test-tail kres test-cpu test-gpu bench clean
