'use strict';
/* The N-API shim's drawListDevice on the CPU (driven by tests/test_draw_list_cpu.py):
 *     node tests/js/draw_list_addon.js <addon.node built from csrc/ht_napi.cc + tests/js/abi_stub.cc + tests/js/draw_list_stub.cc>
 * Successful calls (what reaches the C ABI is in the stub's log) and every malformed call (the message each one throws is printed).
 * ONE device buffer holds all sources, so that the stub can log plane pointers relative to the first entry's.  Prints one JSON line. */
const A = require(process.argv[2]);
const out = { consts: [A.DRAW_RGBA, A.YUV_NV12, A.YUV_I420, typeof A.drawListDevice], thrown: [] };
const c = A.createContext({ cascade: new Uint8Array(64), interval: 5, device: 0 });
A.setGeometry(c, 40, 30, 4, null);
const fb = 40 * 30 * 4;
const src = A.deviceAlloc(c, 100000), dst = A.deviceAlloc(c, 4 * fb + 100), small = A.deviceAlloc(c, 16);
const rgba = { dev: src, offset: 0, width: 7, height: 5, format: A.DRAW_RGBA, matrix: 0, rect: null };                                   /* 140 bytes */
const nv12 = { dev: src, offset: 1001, width: 23, height: 23, format: A.YUV_NV12, matrix: 1, rect: Int32Array.from([1, 1, 21, 21]) };     /* 529 + 288 */
const i420 = { dev: src, offset: 4000, width: 97, height: 81, format: A.YUV_I420, matrix: 3, rect: undefined };                            /* 7857 + 2 * 2009 */
const tail = { dev: src, offset: 100000 - 6, width: 2, height: 2, format: A.YUV_I420 };                                                     /* no offset / matrix / rect given: 6 bytes, the buffer's last */
A.drawListDevice(c, [rgba, nv12, i420, tail], dst, 0);                                   /* the 4-argument form: packed frames at offset 0, no wait */
A.drawListDevice(c, [nv12, { dev: src, width: 7, height: 5, format: A.DRAW_RGBA, offset: undefined }], dst, fb + 48, 4, true);  /* stride, offset, wait; an undefined offset is 0 */
A.drawListDevice(c, [i420], null, 0);                                                     /* the bind form */
function bad(what, fn) { try { fn(); out.thrown.push([what, null]); } catch (e) { out.thrown.push([what, e.constructor.name + ': ' + e.message]); } }
bad('too few arguments', function () { A.drawListDevice(c, [rgba], dst); });
bad('no context', function () { A.drawListDevice(dst, [rgba], dst, 0); });
bad('entries no array', function () { A.drawListDevice(c, rgba, dst, 0); });
bad('no entries', function () { A.drawListDevice(c, [], dst, 0); });
bad('65536 entries', function () { A.drawListDevice(c, new Array(65536).fill(rgba), dst, 0); });
bad('entry no object', function () { A.drawListDevice(c, [rgba, 5], dst, 0); });
bad('entry without dev', function () { A.drawListDevice(c, [{ width: 7, height: 5, format: A.DRAW_RGBA }], dst, 0); });
bad('entry.dev a context', function () { A.drawListDevice(c, [Object.assign({}, rgba, { dev: c })], dst, 0); });
bad('width a string', function () { A.drawListDevice(c, [Object.assign({}, rgba, { width: 'wide' })], dst, 0); });
bad('no format', function () { A.drawListDevice(c, [{ dev: src, width: 7, height: 5 }], dst, 0); });
bad('negative offset', function () { A.drawListDevice(c, [Object.assign({}, rgba, { offset: -4 })], dst, 0); });
bad('rect of three', function () { A.drawListDevice(c, [Object.assign({}, rgba, { rect: Int32Array.from([0, 0, 4]) })], dst, 0); });
bad('rect a plain array', function () { A.drawListDevice(c, [Object.assign({}, rgba, { rect: [0, 0, 4, 4] })], dst, 0); });
bad('frame beyond its buffer', function () { A.drawListDevice(c, [Object.assign({}, tail, { offset: 100000 - 5 })], dst, 0); });
bad('RGBA frame beyond its buffer', function () { A.drawListDevice(c, [Object.assign({}, rgba, { dev: small })], dst, 0); });
bad('zero width', function () { A.drawListDevice(c, [Object.assign({}, rgba, { width: 0 })], dst, 0); });
bad('destination too small', function () { A.drawListDevice(c, [rgba, rgba, rgba, rgba, rgba], dst, 0); });
bad('destination offset beyond', function () { A.drawListDevice(c, [rgba, rgba, rgba, rgba], dst, 0, 104); });
bad('destination stride beyond', function () { A.drawListDevice(c, [rgba, rgba], dst, 4 * fb); });
bad('dst a context', function () { A.drawListDevice(c, [rgba], c, 0); });
bad('stride a string', function () { A.drawListDevice(c, [rgba], dst, 'packed'); });
bad('the library refuses', function () { A.drawListDevice(c, [rgba, rgba, rgba], dst, 0); });
bad('an empty rect is not the whole source', function () { A.drawListDevice(c, [Object.assign({}, rgba, { rect: new Int32Array(4) }), rgba], dst, 0); });
A.destroy(c);
process.stdout.write(JSON.stringify(out) + '\n');
