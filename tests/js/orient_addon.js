'use strict';
/* The N-API shim with ORIENTED formats (an orientation 0..7 in bits 8..10 of the format number), on the CPU (driven by
 * tests/test_orient_bindings_cpu.py):
 *     node tests/js/orient_addon.js <addon.node built from csrc/ht_napi.cc + tests/js/abi_stub.cc + draw_list_stub.cc + ingest_422_stub.cc>
 * The shim sizes and lays a frame out by the BARE format — an oriented YUYV frame is 4 * ceil(w / 2) * h bytes with one plane and an offset
 * that is a multiple of 4, an oriented NV12 frame has its chroma plane behind w * h bytes, an oriented RGBA entry is w * h * 4 bytes — and
 * hands the format number on whole (what reaches the C ABI is in the stubs' logs).  Prints one JSON line. */
const A = require(process.argv[2]);
const out = { thrown: [] };
const c = A.createContext({ cascade: new Uint8Array(64), interval: 5, device: 0 });
A.setGeometry(c, 40, 30, 4, null);
const fb = 40 * 30 * 4, W = 23, H = 7, F = 4 * 12 * 7, F420 = W * H + 2 * 12 * 4;
const fill = function (n) { const a = new Uint8Array(n); for (let i = 0; i < n; i++) a[i] = (i * 7 + 3) & 255; return a; };
function bad(what, fn) { try { fn(); out.thrown.push([what, null]); } catch (e) { out.thrown.push([what, e.constructor.name + ': ' + e.message]); } }
const O = function (k) { return k << 8; };

A.drawFramesYuv(c, fill(2 * F), 2, W, H, A.YUV_YUYV | O(5), 1, null);                        /* exactly fits: sized as 4:2:2 */
A.drawFramesYuv(c, fill(F420), 1, W, H, A.YUV_I420 | O(3), 0, Int32Array.from([0, 0, 7, 23]));  /* a rect of O (7 x 23), outside the stored frame */
bad('host form: oriented yuyv one byte short', function () { A.drawFramesYuv(c, fill(2 * F - 1), 2, W, H, A.YUV_YUYV | O(5), 1, null); });

const src = A.deviceAlloc(c, 8 + 3 * F), dst = A.deviceAlloc(c, 3 * fb);
A.drawFramesYuvDevice(c, src, 8, 3, W, H, A.YUV_UYVY | O(7), 2, 0, null, dst, 0, 0, false);
A.drawFramesYuvDevice(c, src, 1, 1, W, H, A.YUV_NV12 | O(1), 0, 0, null, dst, 0, 0, false);
A.drawFramesYuvDevice(c, src, 2, 1, W, H, A.YUV_I420 | O(6), 3, 0, null, dst, 0, 0, false);
bad('device form: oriented uyvy misaligned offset', function () { A.drawFramesYuvDevice(c, src, 6, 1, W, H, A.YUV_UYVY | O(7), 2, 0, null, dst, 0, 0, false); });
bad('device form: oriented yuyv one byte beyond', function () { A.drawFramesYuvDevice(c, src, 12, 3, W, H, A.YUV_YUYV | O(2), 2, 0, null, dst, 0, 0, false); });

const yuyv = { dev: src, offset: 8, width: W, height: H, format: A.YUV_YUYV | O(1), matrix: 1, rect: Int32Array.from([0, 0, 7, 23]) };
const i420 = { dev: src, offset: 3, width: W, height: H, format: A.YUV_I420 | O(4), matrix: 2, rect: null };
const rgba = { dev: src, offset: 4, width: 5, height: 3, format: A.DRAW_RGBA | O(3), matrix: 0 };
const nv12 = { dev: src, offset: 9, width: 5, height: 3, format: A.YUV_NV12 | O(2), matrix: 0 };
A.drawListDevice(c, [yuyv, i420, rgba, nv12], null, 0);
bad('list entry: oriented rgba one byte beyond', function () { A.drawListDevice(c, [Object.assign({}, rgba, { width: 23, height: 11, offset: 8 + 3 * F - 23 * 11 * 4 + 1 })], dst, 0); });
bad('list entry: oriented yuyv misaligned offset', function () { A.drawListDevice(c, [Object.assign({}, yuyv, { offset: 10 })], dst, 0); });
A.destroy(c);
process.stdout.write(JSON.stringify(out) + '\n');
