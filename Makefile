# Build libqhuff.so (product: HIP kernels for gfx950 + C drop-ins) and the
# oracle's CPU library (test infrastructure).  Used by __graft_entry__.build().
HIPCC   ?= /opt/rocm/bin/hipcc
CC      ?= gcc
ARCH    ?= gfx950
CSRC    := nghttp3_amd/csrc
LIBDIR  := nghttp3_amd/lib
LIB     := $(LIBDIR)/libqhuff.so
ARCHIVE := $(LIBDIR)/libqhuff.a
ORACLE  := oracle/libqh_oracle.so

HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -fvisibility=hidden \
            -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result
CFLAGS   := -std=c11 -O2 -fPIC -fvisibility=hidden -Wall -Wextra

DRIVER  := $(LIBDIR)/qpack

# The host C objects every build of the library links next to its device object.
HOSTOBJS := $(LIBDIR)/qh_scalar.o $(LIBDIR)/qh_qpack.o $(LIBDIR)/qh_http.o $(LIBDIR)/qh_static.o $(LIBDIR)/qh_emit.o $(LIBDIR)/qh_dtset.o $(LIBDIR)/qh_encconn.o $(LIBDIR)/qh_ack.o $(LIBDIR)/qh_blocked.o $(LIBDIR)/qh_partial.o $(LIBDIR)/qh_ustream.o $(LIBDIR)/qh_httpmsg.o $(LIBDIR)/qh_h3.o $(LIBDIR)/qh_h3w.o $(LIBDIR)/qh_h3u.o $(LIBDIR)/qh_h3d.o

all: $(LIB) $(ARCHIVE) $(DRIVER) $(ORACLE)

$(CSRC)/qh_tables.h: nghttp3_amd/tools/gen_tables.py
	python3 nghttp3_amd/tools/gen_tables.py $@

$(LIBDIR)/qh_scalar.o: $(CSRC)/qh_scalar.c $(CSRC)/qh_tables.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_device.o: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(CSRC)/qh_scratch.h $(CSRC)/qh_tables.h $(CSRC)/qh_tokens.h $(CSRC)/qh_qpack_core.h $(CSRC)/qh_emit_core.h $(CSRC)/qh_plan_core.h $(CSRC)/qh_index_core.h $(CSRC)/qh_dtable_core.h $(CSRC)/qh_enc_core.h $(CSRC)/qh_enc_index_core.h $(CSRC)/qh_ack_core.h $(CSRC)/qh_blocked_core.h $(CSRC)/qh_partial_core.h $(CSRC)/qh_ustream_core.h $(CSRC)/qh_http_core.h $(CSRC)/qh_h3_core.h $(CSRC)/qh_h3w_core.h $(CSRC)/qh_h3u_core.h $(CSRC)/qh_h3d_core.h $(CSRC)/qh_frame_fast.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/qh_qpack.o: $(CSRC)/qh_qpack.c $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_static.o: $(CSRC)/qh_static.c $(CSRC)/qh_plan_core.h $(CSRC)/qh_index_core.h $(CSRC)/qh_emit_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_emit.o: $(CSRC)/qh_emit.c $(CSRC)/qh_emit_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_dtset.o: $(CSRC)/qh_dtset.c $(CSRC)/qh_dtable_core.h $(CSRC)/qh_emit_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_encconn.o: $(CSRC)/qh_encconn.c $(CSRC)/qh_enc_core.h $(CSRC)/qh_enc_index_core.h $(CSRC)/qh_index_core.h $(CSRC)/qh_plan_core.h $(CSRC)/qh_dtable_core.h $(CSRC)/qh_emit_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_ack.o: $(CSRC)/qh_ack.c $(CSRC)/qh_ack_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_blocked.o: $(CSRC)/qh_blocked.c $(CSRC)/qh_blocked_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_partial.o: $(CSRC)/qh_partial.c $(CSRC)/qh_partial_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_ustream.o: $(CSRC)/qh_ustream.c $(CSRC)/qh_ustream_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_httpmsg.o: $(CSRC)/qh_httpmsg.c $(CSRC)/qh_http_core.h $(CSRC)/qh_tokens.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_h3.o: $(CSRC)/qh_h3.c $(CSRC)/qh_h3_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_h3w.o: $(CSRC)/qh_h3w.c $(CSRC)/qh_h3w_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_h3u.o: $(CSRC)/qh_h3u.c $(CSRC)/qh_h3u_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_h3d.o: $(CSRC)/qh_h3d.c $(CSRC)/qh_h3d_core.h $(CSRC)/qh_h3_core.h $(CSRC)/qh_qpack_core.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/qh_http.o: $(CSRC)/qh_http.c $(CSRC)/qh_tokens.h include/qhuff.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIB): $(LIBDIR)/qh_device.o $(HOSTOBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

# The QIF bench driver (examples/qpack.cc counterpart), linked against the
# shared library next to it.
$(DRIVER): $(CSRC)/qh_qif.cc include/qhuff.h $(LIB)
	$(CXX) -std=c++17 -O2 -Wall -Wextra -o $@ $< -L$(LIBDIR) -lqhuff \
	  -Wl,-rpath,'$$ORIGIN' -Wl,-rpath-link,/opt/rocm/lib

# Static archive of the same two objects, for linking into libnghttp3 in
# place of the reference's Huffman objects.
$(ARCHIVE): $(LIBDIR)/qh_device.o $(HOSTOBJS)
	rm -f $@
	ar rcs $@ $^

# Phase-timer build for kernel development (not loaded unless QHUFF_LIB
# points at it).
STAMPS := $(LIBDIR)/libqhuff_stamps.so
stamps: $(STAMPS)
$(STAMPS): $(CSRC)/qh_device.hip $(CSRC)/*.inc dev/csrc/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_STAMPS -DQH_STEP_COUNTS=1 -c $< -o $(LIBDIR)/qh_device_stamps.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_stamps.o $(HOSTOBJS)

# Development build (-DQH_DEV_VARIANTS): the product plus the pair decoder
# (dev/csrc/qh_pair_dec.inc: QHUFF_DECODER=pair13...), the segment encoder
# (dev/csrc/qh_enc_seg.inc: QHUFF_SEG=1) and any kPeekVariants entry by name
# (QHUFF_DECODER); loaded only when QHUFF_LIB points at it
# (dev/scripts/dec_variants.py).  The older variants (fsm / fsm2 / lut / run
# / queue decoders, the chunk-engine and streaming encoders, the zero-copy
# host path) and their host side are in the history at 30ebdce; two of their
# kernels (qh_k_enc_lens, qh_k_copy16) still compile here, launched by nothing.
DEV := $(LIBDIR)/libqhuff_dev.so
dev: $(DEV)
$(DEV): $(CSRC)/qh_device.hip $(CSRC)/*.inc dev/csrc/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_DEV_VARIANTS -Idev/csrc -c $< -o $(LIBDIR)/qh_device_dev.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_dev.o $(HOSTOBJS)

# Oracle: -O2 -mavx2 as nghttp3's README.rst:61-67 prescribes for the
# reference build (the Huffman loop itself has no SIMD path).
$(ORACLE): oracle/qh_oracle.c oracle/qh_oracle.h
	$(CC) -std=c11 -O2 -mavx2 -fPIC -shared -pthread -Wall -o $@ $<

# The replay driver on the reference library, when the reference tree is there.
include oracle/ref.mk

clean:
	rm -f $(LIBDIR)/*.o $(DRIVER) $(LIB) $(ARCHIVE) $(STAMPS) $(DEV) $(ORACLE)

.PHONY: all clean stamps

# Fused-encoder ablation builds (timing experiments; wrong bytes):
# make abl ABL=<mask> -> libqhuff_abl<mask>.so (qh_enc_fused.inc QH_EW_ABL)
ABL ?= 0
abl: $(LIBDIR)/libqhuff_abl$(ABL).so
$(LIBDIR)/libqhuff_abl$(ABL).so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_EW_ABL=$(ABL) -c $< -o $(LIBDIR)/qh_device_abl$(ABL).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_abl$(ABL).o $(HOSTOBJS)

# Framing without the LDS stage (development timing: every block parsed from
# global memory at the occupancy registers allow) -> libqhuff_frns.so
frns: $(LIBDIR)/libqhuff_frns.so
$(LIBDIR)/libqhuff_frns.so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_FRAME_NO_STAGE -c $< -o $(LIBDIR)/qh_device_frns.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_frns.o $(HOSTOBJS)

# Count-pass ablations (development timing: make frx FRX=<mask>, see
# QH_FR_ABL in qh_frame.inc) -> libqhuff_frx<mask>.so
frx: $(LIBDIR)/libqhuff_frx$(FRX).so
$(LIBDIR)/libqhuff_frx$(FRX).so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_FR_ABL=$(FRX) -c $< -o $(LIBDIR)/qh_device_frx$(FRX).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_frx$(FRX).o $(HOSTOBJS)

# Length-pass ablations (development timing: make lx LX=<mask>, see
# QH_LX_ABL in qh_lane_enc.inc) -> libqhuff_lx<mask>.so
lx: $(LIBDIR)/libqhuff_lx$(LX).so
$(LIBDIR)/libqhuff_lx$(LX).so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_LX_ABL=$(LX) -c $< -o $(LIBDIR)/qh_device_lx$(LX).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_lx$(LX).o $(HOSTOBJS)

# Codes-pass ablations (development timing: make la LA=<mask>, see QH_LA_ABL
# in qh_lane_enc.inc) -> libqhuff_la<mask>.so
la: $(LIBDIR)/libqhuff_la$(LA).so
$(LIBDIR)/libqhuff_la$(LA).so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_LA_ABL=$(LA) -c $< -o $(LIBDIR)/qh_device_la$(LA).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_la$(LA).o $(HOSTOBJS)

# Dense-pack ablations (development timing: make dp DP=<mask>, see QH_DP_ABL
# in qh_host.inc) -> libqhuff_dp<mask>.so
dp: $(LIBDIR)/libqhuff_dp$(DP).so
$(LIBDIR)/libqhuff_dp$(DP).so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_DP_ABL=$(DP) -c $< -o $(LIBDIR)/qh_device_dp$(DP).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_dp$(DP).o $(HOSTOBJS)

# Phase timers without step counts (development: framing phases, dev/scripts/frame_stamps.py)
frst: $(LIBDIR)/libqhuff_frst.so
$(LIBDIR)/libqhuff_frst.so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_STAMPS -c $< -o $(LIBDIR)/qh_device_frst.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_frst.o $(HOSTOBJS)

# The fused encoder at its free register allocation (3 waves per SIMD), for
# timing against the product's 4 -> libqhuff_ew3.so
ew3: $(LIBDIR)/libqhuff_ew3.so
$(LIBDIR)/libqhuff_ew3.so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_EW_MIN_WAVES=0 -c $< -o $(LIBDIR)/qh_device_ew3.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_ew3.o $(HOSTOBJS)

# Framing count pass with FRC blocks per wave (development timing:
# make frc FRC=16|32) -> libqhuff_frc<FRC>.so
frc: $(LIBDIR)/libqhuff_frc$(FRC).so
$(LIBDIR)/libqhuff_frc$(FRC).so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_FR_COUNT=$(FRC) -c $< -o $(LIBDIR)/qh_device_frc$(FRC).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_frc$(FRC).o $(HOSTOBJS)

# Codes-pass occupancy variants (development timing: make encw5 EW=<waves>
# ES=<stage bytes>) -> libqhuff_ew<EW>s<ES>.so
encw5: $(LIBDIR)/libqhuff_ew$(EW)s$(ES).so
$(LIBDIR)/libqhuff_ew$(EW)s$(ES).so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) -DQH_ENC_WAVES=$(EW) -DQH_ENC_STAGE=$(ES) -c $< -o $(LIBDIR)/qh_device_ew$(EW)s$(ES).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_ew$(EW)s$(ES).o $(HOSTOBJS)

# a build with extra defines: make var V=<name> D="-DQH_...=..."
var: $(LIBDIR)/libqhuff_v$(V).so
$(LIBDIR)/libqhuff_v$(V).so: $(CSRC)/qh_device.hip $(CSRC)/*.inc $(CSRC)/qh_common.h $(HOSTOBJS)
	$(HIPCC) $(HIPFLAGS) $(D) -c $< -o $(LIBDIR)/qh_device_v$(V).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/qh_device_v$(V).o $(HOSTOBJS)
