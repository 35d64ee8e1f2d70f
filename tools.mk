# Native tools: the C host driver (reference argv, GPU search) and the VALU microbenchmark.
HIPCC ?= /opt/rocm/bin/hipcc
CC    ?= gcc
CXX   ?= g++
all: bin/mes_hip bin/mes_seq bin/valu_microbench bin/flow_planes_dump bin/flow_job_dump bin/flow_slim_dump bin/flow_table_dump bin/flow_prebound_dump bin/flow_split_dump

# CPU harness of the row split's rule: lanes -> (list entry, dy rows) (me_geom.h alone)
bin/flow_split_dump: tools/flow_split_dump.cc motionestimation_amd/csrc/me_geom.h
	mkdir -p bin
	$(CXX) -O1 -std=c++17 -Wall -Imotionestimation_amd/csrc -o $@ tools/flow_split_dump.cc

# CPU harness of the launch tile -> job rule (me_geom.h alone)
bin/flow_job_dump: tools/flow_job_dump.cc motionestimation_amd/csrc/me_geom.h
	mkdir -p bin
	$(CXX) -O1 -std=c++17 -Wall -Imotionestimation_amd/csrc -o $@ tools/flow_job_dump.cc

# CPU harness of the flow kernel's LDS item table (me_geom.h alone)
bin/flow_table_dump: tools/flow_table_dump.cc motionestimation_amd/csrc/me_geom.h
	mkdir -p bin
	$(CXX) -O1 -std=c++17 -Wall -Imotionestimation_amd/csrc -o $@ tools/flow_table_dump.cc

# CPU harness of the chain kernel's pre-bound: the cur blocks' addresses and the marker's place (me_geom.h alone)
bin/flow_prebound_dump: tools/flow_prebound_dump.cc motionestimation_amd/csrc/me_geom.h
	mkdir -p bin
	$(CXX) -O1 -std=c++17 -Wall -Imotionestimation_amd/csrc -o $@ tools/flow_prebound_dump.cc

# CPU harness of the box-sum planes' scratch sizing (the planner file alone)
CSRC = motionestimation_amd/csrc
bin/flow_planes_dump: tools/flow_planes_dump.cc $(CSRC)/me_valu_plan.cpp $(CSRC)/me_geom.h $(CSRC)/me_tuning.h
	mkdir -p bin
	$(CXX) -O1 -std=c++17 -Wall -I$(CSRC) -o $@ tools/flow_planes_dump.cc $(CSRC)/me_valu_plan.cpp -lpthread

# CPU harness of the pruning flow launch's two scratch layouts and the bound's plane loads
bin/flow_slim_dump: tools/flow_slim_dump.cc $(CSRC)/me_valu_plan.cpp $(CSRC)/me_geom.h $(CSRC)/me_tuning.h
	mkdir -p bin
	$(CXX) -O1 -std=c++17 -Wall -I$(CSRC) -o $@ tools/flow_slim_dump.cc $(CSRC)/me_valu_plan.cpp -lpthread

bin/mes_hip: tools/mes_main.c include/me.h motionestimation_amd/lib/libme_hip.so
	mkdir -p bin
	$(CC) -O2 -Wall -Iinclude -o $@ tools/mes_main.c -Lmotionestimation_amd/lib -lme_hip \
	    -Wl,-rpath,'$$ORIGIN/../motionestimation_amd/lib' -lm

bin/mes_seq: tools/mes_seq.c include/me.h motionestimation_amd/lib/libme_hip.so
	mkdir -p bin
	$(CC) -O2 -Wall -Iinclude -o $@ tools/mes_seq.c -Lmotionestimation_amd/lib -lme_hip \
	    -Wl,-rpath,'$$ORIGIN/../motionestimation_amd/lib' -lm

bin/valu_microbench: tools/valu_microbench.hip
	mkdir -p bin
	$(HIPCC) --offload-arch=gfx950 -O3 -o $@ $<

.PHONY: all
