# The replay driver on the reference library (oracle/ref_replay.c), built
# into oracle/_ref/ (not committed) when the reference tree is present:
#   make QH_REFERENCE_DIR=/path/to/nghttp3
# Without that directory `make all` builds exactly what it built before.
# Only the QPACK subset of the library and its HTTP message checks
# (lib/nghttp3_http.c) are compiled.  lib/sfparse, which nghttp3_http.c
# includes, is a submodule and may be empty: oracle/shim/sfparse/sfparse.h
# stands in for it and the driver defines its two functions (an empty
# dictionary).  The stand-in is included ahead of every unit and defines the
# parser's own include guard, so a filled submodule is not read either.
QH_REFERENCE_DIR ?= $(wildcard ../reference)
REFOUT      := oracle/_ref
REF_REPLAY  := $(REFOUT)/ref_replay
REF_UNITS   := qpack qpack_huffman qpack_huffman_data buf rcbuf mem ringbuf map ksl str conv vec \
               balloc range objalloc pq unreachable err debug version opl http
REF_DEFS    := -DHAVE_ARPA_INET_H -DHAVE_UNISTD_H -DHAVE_ENDIAN_H -DHAVE_BYTESWAP_H \
               -DHAVE_DECL_BE64TOH=1 -DHAVE_DECL_BSWAP_64=1
# make ref REF_SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
REF_SAN     ?=

ifneq ($(QH_REFERENCE_DIR),)
ifneq ($(wildcard $(QH_REFERENCE_DIR)/lib/nghttp3_qpack.c),)
REF_SRCS := $(foreach u,$(REF_UNITS),$(QH_REFERENCE_DIR)/lib/nghttp3_$(u).c)

all: $(REF_REPLAY)
ref: $(REF_REPLAY)

# nghttp3/version.h from version.h.in, the version read from configure.ac
$(REFOUT)/nghttp3/version.h: $(QH_REFERENCE_DIR)/lib/includes/nghttp3/version.h.in $(QH_REFERENCE_DIR)/configure.ac
	@mkdir -p $(REFOUT)/nghttp3
	v=$$(sed -n 's/^AC_INIT(\[nghttp3\], \[\([0-9.]*\).*/\1/p' $(QH_REFERENCE_DIR)/configure.ac); \
	n=$$(echo $$v | awk -F. '{printf "0x%02x%02x%02x", $$1, $$2, $$3}'); \
	sed -e "s/@PACKAGE_VERSION@/$$v/" -e "s/@PACKAGE_VERSION_NUM@/$$n/" $< > $@

$(REF_REPLAY): oracle/ref_replay.c oracle/shim/sfparse/sfparse.h $(REFOUT)/nghttp3/version.h $(REF_SRCS)
	$(CC) -std=c11 -O1 -g -D_GNU_SOURCE -Wall $(REF_DEFS) $(REF_SAN) -include oracle/shim/sfparse/sfparse.h -Ioracle/shim -I$(REFOUT) \
	  -I$(QH_REFERENCE_DIR)/lib/includes -I$(QH_REFERENCE_DIR)/lib \
	  -o $@ oracle/ref_replay.c $(REF_SRCS)
endif
endif

.PHONY: ref

# (not part of `make clean`: where the reference tree is absent the driver
# cannot be built again)
clean-ref:
	rm -rf $(REFOUT)
.PHONY: clean-ref
