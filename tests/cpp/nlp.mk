# builds the user-NLP device libraries (hipcc, gfx950 cross-compile) and the host-side NLP mirror test (g++):  make -C tests/cpp -f nlp.mk
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)/../..)
HIPCC ?= /opt/rocm/bin/hipcc
all: $(HERE)libuser_nlp.so $(HERE)libuser_nlp_shapes.so $(HERE)nlp_mirror_test
$(HERE)libuser_nlp.so: $(HERE)user_nlp.hip $(wildcard $(ROOT)/polympc_amd/csrc/*.hpp) $(ROOT)/include/polympc/register_nlp.hpp $(ROOT)/include/polympc_amd.h
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -I$(ROOT)/include -o $@ $< -L$(ROOT)/polympc_amd -lpolympc_amd -Wl,-rpath,'$$ORIGIN/../../polympc_amd'
$(HERE)libuser_nlp_shapes.so: $(HERE)user_nlp_shapes.hip $(ROOT)/oracle/nlp_shapes.hpp $(wildcard $(ROOT)/polympc_amd/csrc/*.hpp) $(ROOT)/include/polympc/register_nlp.hpp $(ROOT)/include/polympc_amd.h
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -I$(ROOT)/include -o $@ $< -L$(ROOT)/polympc_amd -lpolympc_amd -Wl,-rpath,'$$ORIGIN/../../polympc_amd'
$(HERE)nlp_mirror_test: $(HERE)nlp_mirror_test.cpp $(ROOT)/include/polympc/polympc.hpp $(HERE)libuser_nlp.so
	g++ -O2 -std=c++14 -Wall -pthread -I$(ROOT)/include -o $@ $< -L$(HERE) -luser_nlp -L$(ROOT)/polympc_amd -lpolympc_amd -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,'$$ORIGIN/../../polympc_amd'
.PHONY: all
