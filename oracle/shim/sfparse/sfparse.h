/* A stand-in for the structured-field parser that the reference's
 * lib/nghttp3_http.c includes (lib/sfparse is a submodule of the reference
 * tree and may be empty).  It declares the names that file uses and nothing
 * else; oracle/ref_replay.c defines the two functions, and its dictionary is
 * always empty.  The replay driver is built with this header even where the
 * reference tree has the submodule, so that a transcript does not depend on
 * it (oracle/README.md: what the transcripts do not judge). */
#ifndef QH_ORACLE_SHIM_SFPARSE_H
#define QH_ORACLE_SHIM_SFPARSE_H
/* (the parser's own guard: oracle/ref.mk includes this file ahead of every
 * unit, so a copy of the parser beside nghttp3_http.c reads as empty) */
#ifndef SFPARSE_H
#  define SFPARSE_H
#endif

#include <stddef.h>
#include <stdint.h>

#define SFPARSE_ERR_EOF (-2)

typedef enum sfparse_type {
  SFPARSE_TYPE_BOOLEAN,
  SFPARSE_TYPE_INTEGER
} sfparse_type;

typedef struct sfparse_vec {
  uint8_t *base;
  size_t len;
} sfparse_vec;

typedef struct sfparse_value {
  sfparse_type type;
  int boolean;
  int64_t integer;
} sfparse_value;

typedef struct sfparse_parser {
  const uint8_t *pos;
  const uint8_t *end;
} sfparse_parser;

void sfparse_parser_init(sfparse_parser *sfp, const uint8_t *data, size_t datalen);
int sfparse_parser_dict(sfparse_parser *sfp, sfparse_vec *dest_key, sfparse_value *dest_value);

#endif
